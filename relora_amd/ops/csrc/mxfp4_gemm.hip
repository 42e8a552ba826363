// Some packed-fp32 instruction forms miscompute on this target, so this file
// is compiled without them (as fp8_gemm.hip; the attribute has to cover the
// headers too, or their helpers are not inlined and the accumulators spill).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "hip/hip_runtime.h"
// MXFP4 frozen-W path (`--quantize mxfp4`) on the gfx950 block-scaled matrix
// cores.
//
// Format (ops/quant.py quantize_mxfp4_ref is the definition): OCP MX, a block
// is 32 consecutive k of one row of W [N,K].  Per block one E8M0 scale byte
//   byte = clamp(E - 2, 0, 254),  E = biased fp32 exponent field of amax
// (127 for an all-zero block), so amax * 2^(127-byte) lies in [4, 8); per
// element one e2m1 code (sign in bit 3, magnitudes 0 .5 1 1.5 2 3 4 6) of
// v * 2^(127-byte), rounded to nearest with ties to the even code, saturating
// at 6.  The sign bit of v is always kept (so -0 and values that round to
// zero encode as code 8).  Two codes a byte, the LOW nibble is the lower k.
// codes uint8 [N, Kp/2], scales uint8 [N, Kp/32], Kp = K rounded up to 32;
// padding of a short last block encodes as zero codes.
// value = e2m1(code) * 2^(byte-127).
//
//   quantize_rows_mxfp4    bf16 [R,K] -> (codes, scales)
//   dequantize_rows_mxfp4  codes, scales -> bf16 | fp32 [R,K]
//   fused_mxfp4_gemm       y = (xq·W4^T)·sx (+bias) + s·t·Bw^T, bf16 out,
//                          xq/xs from quantize_rows_fp8, W4 as stored
//   ..._ragged             any N (out_features) and any K (in_features): xq/xs
//                          from quantize_rows_fp8_padded when K % 128 != 0
//   fused_mxfp4_gemm_dx    dx = dy @ W on the fp8 cores, W transcoded to e4m3
//                          per stripe while staged (at the end of this file)
//
// GEMM structure: fused_fp8_gemm's 256x256 tile, 8 waves (2M x 4N),
// double-buffered global_load_lds staging, XCD remap and one vmcnt(0) +
// barrier per 128-k tile, with what the format changes:
//   * v_mfma_scale_f32_16x16x128_f8f6f4 with A = e4m3 (cbsz 0), B = e2m1
//     (blgp 4) and a per-lane E8M0 scale on B; A's scale is the constant 127.
//   * Lane-to-k assignment, as the read-back test found it on the hardware:
//     a 4-bit operand's lane (fr, fq) holds k = 32*fq .. 32*fq+31 in its 4
//     dwords, low nibble first, and its scale byte covers exactly those 32 k
//     (one MX block); an 8-bit operand's lane holds k = 16*fq .. +15 in
//     dwords 0-3 and k = 64+16*fq .. +15 in dwords 4-7.  So the e2m1 lane
//     reads the 16-byte chunk fq of its 64-byte row, and the e4m3 lane the
//     chunks fq and 4+fq of its 128-byte row: fp8_gemm's assignment is the
//     hardware's own order, and its swizzle (chunk ^= (row>>1)&7) carries
//     over to the A image and to the bf16 LoRA fragments that reuse it.  The
//     B image is 2-way conflicted when linear (rows 0-3 and 12-15 of a b128
//     service group share bank slots); chunk ^= 2*row[3] makes it
//     conflict-free in tools/lds_bank_model.py (mxfp4_gemm_b_frag_reads).
//   * The B tile is 16 KiB, the double buffer 96 KiB; a B fragment is 4
//     dwords, the four resident ones cost 16 VGPRs.
//   * Scales: one dword per (W row, K-tile) holds the tile's four block
//     bytes.  A lane loads the dwords of its 4 column fragments one tile
//     ahead (L2 hits) and shifts byte fq down itself, since the instruction's
//     byte selector is an immediate.
// Epilogue as fused_fp8_gemm: acc * xs[m]/448 (no W row scale), the rank-r
// bf16 MFMA update on the same accumulators, bias, one rounding to bf16, b128
// row stores through LDS (in two 64-row halves: 96 KiB hold 8 x 8 KiB).
//
// The device code here has copies of its own of what gemm_tile.h shares
// between the bf16 kernels (XCD remap, coordinates, the stagers, the LoRA
// update); only the host preparation (gemm_host.h) is shared.  Moving this
// kernel onto shared pieces changes its instruction order, and a shift of
// under 1 % cannot be judged with tools/bench_fp8_gemm.py, which times
// identical code up to 1.5 % apart between two builds (the kernels timed next
// to it differ).  fused_fp8_gemm, measured alone, did lose 1.4 % that way
// (profiles/stage19_gemm_shared.md), so this file was left as it was.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"
#include "gemm_host.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_m;
typedef __attribute__((ext_vector_type(4))) float f32x4_m;
typedef __attribute__((ext_vector_type(4))) int i32x4_m;
typedef __attribute__((ext_vector_type(8))) int i32x8_m;

#define MX_BLOCK 32
#define E4M3_MAX 448.0f

// ---------------------------------------------------------------------------
// Quantiser / dequantiser
// ---------------------------------------------------------------------------

// scale byte of a block from its amax (>= 0)
DEV_INLINE unsigned mx_scale_byte(float amax) {
  if (!(amax > 0.f)) return 127u;
  const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 2;
  return (unsigned)min(max(e, 0), 254);
}

// 2^(127-byte): a normal fp32 for every byte mx_scale_byte returns (<= 253)
DEV_INLINE float mx_inv_scale(unsigned byte) { return __uint_as_float((254u - byte) << 23); }

// 2^(byte-127); byte 0 is the fp32 subnormal 2^-127
DEV_INLINE float mx_scale(unsigned byte) {
  return __uint_as_float(byte ? byte << 23 : 0x00400000u);
}

// e2m1 code of s (already scaled): RNE on the magnitude grid, ties to the
// even code, saturating; the sign bit of s is kept.
DEV_INLINE unsigned e2m1_encode(float s) {
  const float a = fabsf(s);
  const unsigned m = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                     (a >= 3.5f) + (a > 5.0f);
  return m | ((__float_as_uint(s) >> 28) & 8u);
}

DEV_INLINE float e2m1_decode(unsigned c) {
  const unsigned m = c & 7u;
  const float mag = m < 2u ? 0.5f * (float)m
                           : __uint_as_float((((m >> 1) + 126u) << 23) | ((m & 1u) << 22));
  return (c & 8u) ? -mag : mag;
}

// K % 32 == 0: four lanes per block, 8 bf16 (one 16-byte load) per lane, the
// block max by two shuffles, one dword of 8 codes per lane; consecutive lanes
// load and store consecutive memory.  n8 = R*K/8 lanes.
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(
    const __hip_bfloat16* __restrict__ x, uint8_t* __restrict__ codes,
    uint8_t* __restrict__ scales, long n8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n8;  // n8 % 4 == 0: a 4-lane group is live or dead as one
  const uint4 u = live ? reinterpret_cast<const uint4*>(x)[i] : make_uint4(0, 0, 0, 0);
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
  float v[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(w[j] << 16);
    v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(v[j]));
  am = fmaxf(am, __shfl_xor(am, 1));
  am = fmaxf(am, __shfl_xor(am, 2));
  if (!live) return;
  const unsigned byte = mx_scale_byte(am);
  const float inv = mx_inv_scale(byte);
  unsigned packed = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) packed |= e2m1_encode(__fmul_rn(v[j], inv)) << (4 * j);
  reinterpret_cast<unsigned*>(codes)[i] = packed;
  if ((i & 3) == 0) scales[i >> 2] = (uint8_t)byte;
}

// any K (e.g. 5461): one thread per block, scalar loads, byte stores; the
// last block of a row may be short, its padding gives zero codes.  Off the
// hot path (once per merge).
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_any_kernel(
    const __hip_bfloat16* __restrict__ x, uint8_t* __restrict__ codes,
    uint8_t* __restrict__ scales, long nblocks, int K, int bpr) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const long row = b / bpr;
  const int k0 = (int)(b % bpr) * MX_BLOCK;
  const int len = min(MX_BLOCK, K - k0);
  const __hip_bfloat16* src = x + row * K + k0;
  float am = 0.f;
  for (int k = 0; k < len; ++k) am = fmaxf(am, fabsf(to_f32(src[k])));
  const unsigned byte = mx_scale_byte(am);
  const float inv = mx_inv_scale(byte);
  uint8_t* dst = codes + b * (MX_BLOCK / 2);
  for (int k = 0; k < MX_BLOCK; k += 2) {
    const unsigned lo = k < len ? e2m1_encode(__fmul_rn(to_f32(src[k]), inv)) : 0u;
    const unsigned hi = k + 1 < len ? e2m1_encode(__fmul_rn(to_f32(src[k + 1]), inv)) : 0u;
    dst[k >> 1] = (uint8_t)(lo | (hi << 4));
  }
  scales[b] = (uint8_t)byte;
}

std::vector<torch::Tensor> quantize_rows_mxfp4(torch::Tensor x) {
  const char* fn = "quantize_rows_mxfp4";
  TORCH_CHECK(x.is_cuda(), fn, ": x must be a GPU tensor");
  TORCH_CHECK(x.dim() == 2, fn, ": x must be 2-D [R, K]");
  TORCH_CHECK(x.is_contiguous(), fn, ": x must be contiguous");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, fn, ": x must be bf16");
  const long R = x.size(0), K = x.size(1);
  TORCH_CHECK(R > 0 && K > 0, fn, ": R and K must be > 0");
  TORCH_CHECK(K < (1L << 31) - MX_BLOCK && R < (1L << 31), fn, ": shape too large");
  const long bpr = (K + MX_BLOCK - 1) / MX_BLOCK;  // blocks per row
  auto codes = torch::empty({R, bpr * (MX_BLOCK / 2)}, x.options().dtype(torch::kUInt8));
  auto scales = torch::empty({R, bpr}, x.options().dtype(torch::kUInt8));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const auto* xp = (const __hip_bfloat16*)x.data_ptr();
  if (K % MX_BLOCK == 0) {
    const long n8 = R * K / 8;
    hipLaunchKernelGGL(quantize_rows_mxfp4_kernel, dim3((unsigned)((n8 + 255) / 256)),
                       dim3(256), 0, stream, xp, codes.data_ptr<uint8_t>(),
                       scales.data_ptr<uint8_t>(), n8);
  } else {
    const long nblocks = R * bpr;
    hipLaunchKernelGGL(quantize_rows_mxfp4_any_kernel,
                       dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, stream, xp,
                       codes.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>(), nblocks, (int)K,
                       (int)bpr);
  }
  HIP_CHECK_LAST();
  return {codes, scales};
}

// VEC (K % 32 == 0, so rows are dense in codes and scales): one thread per
// dword of 8 codes.  Otherwise one thread per output element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dequantize_rows_mxfp4_kernel(
    const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales,
    T* __restrict__ out, long n, int K, int bpr) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    if (i >= n / 8) return;
    const unsigned c = reinterpret_cast<const unsigned*>(codes)[i];
    const float sc = mx_scale(scales[i >> 2]);
    T v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = from_f32<T>(__fmul_rn(e2m1_decode(c >> (4 * j)), sc));
    store8(out + i * 8, *reinterpret_cast<const Vec8<T>*>(v));
  } else {
    if (i >= n) return;
    const long row = i / K;
    const int k = (int)(i % K);
    const unsigned c = codes[row * bpr * (MX_BLOCK / 2) + (k >> 1)] >> (4 * (k & 1));
    out[i] = from_f32<T>(__fmul_rn(e2m1_decode(c), mx_scale(scales[row * bpr + k / MX_BLOCK])));
  }
}

torch::Tensor dequantize_rows_mxfp4(torch::Tensor codes, torch::Tensor scales, long R, long K,
                                    torch::ScalarType dtype) {
  const char* fn = "dequantize_rows_mxfp4";
  TORCH_CHECK(codes.is_cuda(), fn, ": codes must be a GPU tensor");
  TORCH_CHECK(codes.scalar_type() == torch::kUInt8 && codes.is_contiguous(), fn,
              ": codes must be contiguous uint8");
  TORCH_CHECK(R > 0 && K > 0 && K < (1L << 31) - MX_BLOCK, fn, ": bad R or K");
  const long bpr = (K + MX_BLOCK - 1) / MX_BLOCK;
  TORCH_CHECK(codes.numel() == R * bpr * (MX_BLOCK / 2), fn,
              ": codes must hold R*Kp/2 bytes (Kp = K rounded up to 32)");
  TORCH_CHECK(scales.device() == codes.device() && scales.scalar_type() == torch::kUInt8 &&
                  scales.is_contiguous() && scales.numel() == R * bpr,
              fn, ": scales must be R*Kp/32 contiguous uint8 values on the codes' device");
  TORCH_CHECK(dtype == torch::kBFloat16 || dtype == torch::kFloat32, fn,
              ": output dtype must be bf16 or fp32");
  auto out = torch::empty({R, K}, codes.options().dtype(dtype));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const long n = R * K;
  const bool vec = K % MX_BLOCK == 0;
  const long threads = vec ? n / 8 : n;
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  const uint8_t* cp = codes.data_ptr<uint8_t>();
  const uint8_t* sp = scales.data_ptr<uint8_t>();
#define LAUNCH_DQ(T, PTR, V)                                                           \
  hipLaunchKernelGGL((dequantize_rows_mxfp4_kernel<T, V>), grid, block, 0, stream, cp, \
                     sp, PTR, n, (int)K, (int)bpr)
  if (dtype == torch::kBFloat16) {
    auto* op = (__hip_bfloat16*)out.data_ptr();
    if (vec) LAUNCH_DQ(__hip_bfloat16, op, true); else LAUNCH_DQ(__hip_bfloat16, op, false);
  } else {
    auto* op = out.data_ptr<float>();
    if (vec) LAUNCH_DQ(float, op, true); else LAUNCH_DQ(float, op, false);
  }
#undef LAUNCH_DQ
  HIP_CHECK_LAST();
  return out;
}

// ---------------------------------------------------------------------------
// fused_mxfp4_gemm
// ---------------------------------------------------------------------------

// Swizzles on a byte offset within an image; both keep the row and are
// involutions, so one function maps LDS byte -> source byte when staging and
// logical byte -> LDS byte when reading.
// A-type image [rows][128 B]: 16-byte chunk (bits 4..6) ^= (row>>1)&7, as fp8_gemm
DEV_INLINE unsigned swz_a(unsigned o) { return o ^ (((o >> 8) & 7u) << 4); }
// B image [rows][64 B]: 16-byte chunk (bits 4..5) ^= 2*row[3]
DEV_INLINE unsigned swz_b(unsigned o) { return o ^ (((o >> 9) & 1u) << 5); }

// Stage one [256][128 B] tile (32 KiB) via glds: 32 wave-level 1-KiB pieces
// (8 full rows each), 4 per wave.  The LDS image is lane-linear as glds
// requires; the per-lane GLOBAL source address carries the swizzle.
// CLAMP: rows past `last` read row `last` instead (the edge tile of a ragged
// operand: nothing outside the allocation is touched, the image rows feed
// accumulators nobody stores).
template <bool CLAMP = false>
DEV_INLINE void stage_a_tile(char* image, const char* gbase, long row0, long ld, long k0,
                             int wave, int lane, long last = 0) {
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) {
    const int piece = wave * 4 + p4;
    const unsigned s = swz_a(piece * 1024u + lane * 16u);  // source byte in tile
    long row = row0 + (s >> 7);
    if (CLAMP) row = row < last ? row : last;
    const char* src = gbase + row * ld + k0 + (s & 127u);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// Stage one [256][64 B] e2m1 tile (16 KiB): 16 pieces of 16 full rows, 2 per wave
DEV_INLINE void stage_b_tile(char* image, const char* gbase, long row0, long ld, long k0,
                             int wave, int lane) {
#pragma unroll
  for (int p2 = 0; p2 < 2; ++p2) {
    const int piece = wave * 2 + p2;
    const unsigned s = swz_b(piece * 1024u + lane * 16u);
    const char* src = gbase + (row0 + (s >> 6)) * ld + k0 + (s & 63u);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// The same for a ragged W: rows past `last` read row `last`; with KRAG a row
// of the tile holds only `nbt` 16-byte chunks (the MX blocks that exist in the
// last 128-k tile of a row of pitch Kp/2), and a lane whose swizzled source
// chunk lies behind them reads the row's last existing chunk instead.  Those
// codes are finite (e2m1 has no NaN), get the scale byte 127 and meet the zero
// codes of xq's pad.  Rows of pitch Kp/2 are multiples of 16 bytes, so glds
// sources them at any K.
template <bool KRAG>
DEV_INLINE void stage_b_tile_edge(char* image, const char* gbase, long row0, long ld, long k0,
                                  int wave, int lane, long last, int nbt) {
#pragma unroll
  for (int p2 = 0; p2 < 2; ++p2) {
    const int piece = wave * 2 + p2;
    const unsigned s = swz_b(piece * 1024u + lane * 16u);
    long row = row0 + (s >> 6);
    row = row < last ? row : last;
    unsigned col = s & 63u;
    if (KRAG) col = min(col, (unsigned)(nbt - 1) * 16u);
    const char* src = gbase + row * ld + k0 + col;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// a dword of scale bytes from any byte address (global memory takes it)
DEV_INLINE unsigned load_u32_any(const char* p) {
  unsigned v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// e4m3 A fragment: k = 16*fq .. +15 and 64+16*fq .. +15 of `row` (chunks fq, 4+fq)
DEV_INLINE i32x8_m frag_e4m3(const char* image, int row, int fq) {
  const unsigned p = swz_a((unsigned)row * 128u + (unsigned)fq * 16u);
  const i32x4_m lo = *reinterpret_cast<const i32x4_m*>(image + p);
  const i32x4_m hi = *reinterpret_cast<const i32x4_m*>(image + (p ^ 64u));
  return i32x8_m{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// e2m1 B fragment: the 32 codes k = 32*fq .. +31 of `row` (chunk fq)
DEV_INLINE i32x4_m frag_e2m1(const char* image, int row, int fq) {
  return *reinterpret_cast<const i32x4_m*>(image + swz_b((unsigned)row * 64u + (unsigned)fq * 16u));
}

// bf16 fragment of an A-type image (16x16x32: row l&15, 8 k at ks*32+(l>>4)*8)
DEV_INLINE bf16x8_m frag_bf16_a(const char* image, int row, int ks, int fq) {
  const unsigned o = (unsigned)row * 128u + (unsigned)ks * 64u + (unsigned)fq * 16u;
  return *reinterpret_cast<const bf16x8_m*>(image + swz_a(o));
}

#define MX_A_BYTES (256 * 128)
#define MX_B_BYTES (256 * 64)
#define MX_BUF_A(b) (smem + (b) * (MX_A_BYTES + MX_B_BYTES))
#define MX_BUF_B(b) (smem + (b) * (MX_A_BYTES + MX_B_BYTES) + MX_A_BYTES)
#define MX_SMEM_BYTES (2 * (MX_A_BYTES + MX_B_BYTES))  // 96 KiB

// RAGGED: any N >= 1.  The grid has ceil(N/256) block columns; in the last one
// every W-side row index >= N (B tile, bw tile, scale row, bias) is clamped to
// N-1, and the epilogue stores rows of pitch N up to column N only.  The scale
// dwords are addressed by byte (base + 32-bit lane offset) and may be unaligned.
// KRAG (with RAGGED): any K >= 1 as well.  xq has pitch Kp128 = K rounded up to
// 128 with zero codes in [K, Kp128) (quantize_rows_fp8_padded); wq has pitch
// Kp/2 and wsc bpr = ceil(K/32) bytes a row, Kp = K rounded up to 32.  The last
// tile of a row holds nb = bpr - 4*(KT-1) blocks (1..4): its code chunks past
// nb are clamped in stage_b_tile_edge, its scale dword is loaded END-aligned
// (the four bytes that end with the row, so nothing behind the row, for the
// last row nothing behind wsc, is read), shifted down, and the bytes of the
// missing blocks are set to 127: 0xFF is NaN in E8M0 and must not reach the
// matrix instruction.  A row shorter than a dword (K <= 96) loads byte by byte.
template <bool RAGGED, bool KRAG>
__global__ __launch_bounds__(512) void fused_mxfp4_gemm_kernel(
    const uint8_t* __restrict__ xq,         // [M,K] e4m3 codes ([M,Kp128] with KRAG)
    const float* __restrict__ xa,           // [M] absmax of x rows
    const uint8_t* __restrict__ wq,         // [N,K/2] e2m1 codes ([N,Kp/2] with KRAG)
    const unsigned* __restrict__ wsc,       // [N,K/128] dwords of 4 E8M0 bytes ([N,bpr] bytes)
    const __hip_bfloat16* __restrict__ t,   // [M,r] or null (pre-scaled)
    const __hip_bfloat16* __restrict__ bw,  // [N,r] or null
    const __hip_bfloat16* __restrict__ bias,  // [N] or null
    __hip_bfloat16* __restrict__ y,         // [M,N]
    long M, long N, long K, int r) {
  // one __shared__ array only (glds pipeline rule)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][A 32K | B 16K]

  // XCD-aware blockIdx remap (bijective form), as in fused_lora_gemm
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbn = (int)((RAGGED ? N + 255 : N) >> 8);
  const long m0 = (long)(wgid / nbn) << 8;
  const long n0 = (long)(wgid % nbn) << 8;
  const long nl = N - 1;  // last row of W (RAGGED clamps to it)

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 2;   // 0..1: wave m-position (128 rows)
  const int wc = wave & 3;    // 0..3: wave n-position (64 cols)
  const int fr = lane & 15;   // fragment row / C column
  const int fq = lane >> 4;   // fragment k-group (= MX block of the tile) / C row group

  f32x4_m acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_m{0.f, 0.f, 0.f, 0.f};

  const char* xg = (const char*)xq;
  const char* wg = (const char*)wq;
  const long KA = KRAG ? (K + 127) & ~127L : K;         // pitch of xq, reduction depth
  const int bpr = (int)(KRAG ? (K + 31) >> 5 : K >> 5);  // scale bytes per W row
  const long ldw = KRAG ? (long)bpr * 16 : K >> 1;       // W row pitch in bytes
  const int KT = (int)(KA >> 7);     // 128-k tiles (= scale dwords per W row unless KRAG)
  const int nb = KRAG ? bpr - 4 * (KT - 1) : 4;          // blocks in a row's last tile
  // this lane's 4 scale rows (one per column fragment), tile 0
  const unsigned* srow = wsc + (n0 + wc * 64 + fr) * KT;
  // RAGGED: byte offsets of the (clamped) rows from row n0, 32-bit next to a
  // scalar base
  const char* sbase = (const char*)wsc + n0 * bpr;
  unsigned so[4];
  unsigned sc[4];
  if (RAGGED) {
    const int nrel = (int)(nl - n0 < 255 ? nl - n0 : 255);
#pragma unroll
    for (int j = 0; j < 4; ++j) so[j] = (unsigned)min(wc * 64 + j * 16 + fr, nrel) * (unsigned)bpr;
    if (KRAG && bpr < 4) {  // K <= 96: one tile, the row is shorter than a dword
      const unsigned fill = 0x7f7f7f7fu << (8 * bpr);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned w = fill;
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (e < bpr) w |= (unsigned)(uint8_t)sbase[so[j] + e] << (8 * e);
        sc[j] = w;
      }
    } else {  // tile 0 is whole, or the only one with bpr == 4
#pragma unroll
      for (int j = 0; j < 4; ++j) sc[j] = load_u32_any(sbase + so[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j] = srow[(long)j * 16 * KT];
  }

  stage_a_tile(MX_BUF_A(0), xg, m0, KA, 0, wave, lane);
  if (RAGGED)
    stage_b_tile_edge<KRAG>(MX_BUF_B(0), wg, n0, ldw, 0, wave, lane, nl, KT == 1 ? nb : 4);
  else
    stage_b_tile(MX_BUF_B(0), wg, n0, ldw, 0, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    unsigned nsc[4] = {0u, 0u, 0u, 0u};
    unsigned fix_sh = 0u, fix_or = 0u;  // KRAG: applied to the next tile's scale dwords once landed
    if (kt + 1 < KT) {
      stage_a_tile(MX_BUF_A(cur ^ 1), xg, m0, KA, (long)(kt + 1) << 7, wave, lane);
      if (RAGGED) {
        const bool lastn = KRAG && kt + 2 == KT;  // uniform: the next tile is the last
        stage_b_tile_edge<KRAG>(MX_BUF_B(cur ^ 1), wg, n0, ldw, (long)(kt + 1) << 6, wave, lane,
                                nl, lastn ? nb : 4);
        // two tiles: bpr >= 5, so the dword that ends with the row starts in it
        const char* sp = sbase + (lastn ? bpr - 4 : 4 * (kt + 1));
        if (lastn && nb < 4) {
          fix_sh = 8u * (unsigned)(4 - nb);
          fix_or = 0x7f7f7f7fu << (8 * nb);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) nsc[j] = load_u32_any(sp + so[j]);
      } else {
        stage_b_tile(MX_BUF_B(cur ^ 1), wg, n0, ldw, (long)(kt + 1) << 6, wave, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) nsc[j] = srow[(long)j * 16 * KT + kt + 1];
      }
    }
    const char* A = MX_BUF_A(cur);
    const char* B = MX_BUF_B(cur);
    __builtin_amdgcn_s_setprio(1);
    // the 4 B fragments (16 VGPRs) and their block scales stay resident
    i32x8_m bf[4];
    int sb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x4_m b4 = frag_e2m1(B, wc * 64 + j * 16 + fr, fq);
      bf[j] = i32x8_m{b4[0], b4[1], b4[2], b4[3], 0, 0, 0, 0};
      sb[j] = (int)((sc[j] >> (8 * fq)) & 0xffu);  // byte fq -> byte 0 (op-sel 0)
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const i32x8_m af = frag_e4m3(A, wr * 128 + i * 16 + fr, fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            af, bf[j], acc[i][j], 0 /*A e4m3*/, 4 /*B e2m1*/, 0, 127 /*A scale 2^0*/, 0, sb[j]);
    }
    __builtin_amdgcn_s_setprio(0);
    // drain next tile's glds and scale loads, then release the buffers
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) sc[j] = KRAG ? (nsc[j] >> fix_sh) | fix_or : nsc[j];
  }

  // ---- 1. activation row scale on the resident accumulators (fp32) -------
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4_m ax = *reinterpret_cast<const f32x4_m*>(xa + m0 + wr * 128 + i * 16 + fq * 4);
    const f32x4_m sx = {__fdiv_rn(ax[0], E4M3_MAX), __fdiv_rn(ax[1], E4M3_MAX),
                        __fdiv_rn(ax[2], E4M3_MAX), __fdiv_rn(ax[3], E4M3_MAX)};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] * sx;
  }

  // ---- 2. LoRA rank-r update: acc += t_s-tile @ Bw-tile^T (bf16 MFMA) -----
  // t and Bw chunks are [256][64] bf16 = A-type images at smem and smem+32K
  if (r > 0) {
    const int RC = r >> 6;
    const long ldr = (long)r * 2;
    char* TA = smem;
    char* TB = smem + MX_A_BYTES;
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_a_tile(TA, (const char*)t, m0, ldr, (long)c << 7, wave, lane);
      stage_a_tile<RAGGED>(TB, (const char*)bw, n0, ldr, (long)c << 7, wave, lane, nl);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_m bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = frag_bf16_a(TB, wc * 64 + j * 16 + fr, ks, fq);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bf16x8_m afr = frag_bf16_a(TA, wr * 128 + i * 16 + fr, ks, fq);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[j], acc[i][j],
                                                                0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();  // all waves done reading before the next chunk lands
    }
  }

  // ---- 3+4. bias, one bf16 rounding, b128 row stores through LDS ----------
  // each wave owns 8 KiB: its 128x64 tile goes out in two 64-row halves
  __bf16* mine = (__bf16*)smem + wave * (64 * 64);
  float bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    long n = n0 + wc * 64 + j * 16 + fr;
    if (RAGGED) n = n < nl ? n : nl;
    bv[j] = bias ? (float)bias[n] : 0.f;
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = i4 * 16 + fq * 4 + reg;  // within the half
          const int col = j * 16 + fr;
          mine[row * 64 + col] = (__bf16)(acc[half * 4 + i4][j][reg] + bv[j]);
        }
    // no block barrier: a wave reads only its own region; keep the order
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int row = rr * 8 + (lane >> 3);          // 0..63
      const int cb = (lane & 7) * 8;                 // 8-col chunk
      const bf16x8_m vv = *reinterpret_cast<const bf16x8_m*>(mine + row * 64 + cb);
      if (RAGGED) {
        // pitch N: with N % 8 != 0 a row start is only 2-byte aligned, so the
        // 16-byte store goes through Vec8 (alignof 2); the chunk that straddles
        // N goes element by element, later ones are skipped
        const long col = n0 + wc * 64 + cb;
        __hip_bfloat16* dst = y + (m0 + wr * 128 + half * 64 + row) * N + col;
        if (col + 8 <= N) {
          store8(dst, *reinterpret_cast<const Vec8<__hip_bfloat16>*>(&vv));
        } else {
          const __hip_bfloat16* sv = reinterpret_cast<const __hip_bfloat16*>(&vv);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (col + e < N) dst[e] = sv[e];
        }
      } else {
        *reinterpret_cast<bf16x8_m*>(y + (m0 + wr * 128 + half * 64 + row) * N + n0 + wc * 64 +
                                     cb) = vv;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

static void check_mx_u8(const char* fn, const char* what, const torch::Tensor& v,
                        const torch::Device& dev, long numel, const char* count) {
  TORCH_CHECK(v.is_cuda() && v.device() == dev, fn, ": ", what, " must be on xq's GPU");
  TORCH_CHECK(v.scalar_type() == torch::kUInt8, fn, ": ", what, " must be uint8");
  TORCH_CHECK(v.is_contiguous(), fn, ": ", what, " must be contiguous");
  TORCH_CHECK(v.numel() == numel, fn, ": ", what, " must hold ", count, " bytes");
  // 16-byte glds pieces and the scale dwords: a byte-offset view would misalign them
  TORCH_CHECK((uintptr_t)v.data_ptr() % 16 == 0, fn, ": ", what, " must be 16-byte aligned");
}

// xq / xs as quantize_rows_fp8 returns them (the kernel divides xs by 448);
// wq / wscales as quantize_rows_mxfp4 returns them for a [N,K] weight.
torch::Tensor fused_mxfp4_gemm(torch::Tensor xq, torch::Tensor xs, torch::Tensor wq,
                               torch::Tensor wscales, long N, torch::Tensor t,
                               torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_mxfp4_gemm";
  TORCH_CHECK(xq.is_cuda(), fn, ": xq must be a GPU tensor");
  TORCH_CHECK(xq.dim() == 2, fn, ": xq must be 2-D [M, K]");
  const long M = xq.size(0), K = xq.size(1);
  TORCH_CHECK(M > 0 && K > 0 && N > 0, fn, ": M, N and K must be > 0");
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 128 == 0, fn,
              " requires M%256==0, N%256==0, K%128==0");
  TORCH_CHECK(M * N < (1L << 40) && K < (1L << 31), fn, ": shape too large");
  const auto dev = xq.device();
  check_mx_u8(fn, "x codes", xq, dev, M * K, "M*K");
  TORCH_CHECK(xs.device() == dev, fn, ": x absmax must be on xq's device");
  TORCH_CHECK(xs.scalar_type() == torch::kFloat32, fn, ": x absmax must be fp32");
  TORCH_CHECK(xs.is_contiguous(), fn, ": x absmax must be contiguous");
  TORCH_CHECK(xs.numel() == M, fn, ": x absmax must hold one value per row");
  check_mx_u8(fn, "w codes", wq, dev, N * K / 2, "N*K/2");
  check_mx_u8(fn, "w scales", wscales, dev, N * K / MX_BLOCK, "N*K/32");
  const LoraArgs a = prep_lora_bias(fn, "xq", dev, t, bw, bias, M, N, 64, 256, lora_scale);
  auto y = torch::empty({M, N}, xq.options().dtype(torch::kBFloat16));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((unsigned)((M >> 8) * (N >> 8))), block(512);
  hipLaunchKernelGGL((fused_mxfp4_gemm_kernel<false, false>), grid, block, MX_SMEM_BYTES, stream,
                     xq.data_ptr<uint8_t>(), xs.data_ptr<float>(), wq.data_ptr<uint8_t>(),
                     (const unsigned*)wscales.data_ptr<uint8_t>(),
                     a.t, a.bw, a.bias, (__hip_bfloat16*)y.data_ptr(), M, N, K, a.r);
  HIP_CHECK_LAST();
  return y;
}

// one uint8 operand of fused_mxfp4_gemm_ragged; `align` 1 for none
static void check_mx_u8_ragged(const char* fn, const char* what, const torch::Tensor& v,
                               const torch::Device& dev, long numel, const char* count,
                               int align) {
  TORCH_CHECK(v.is_cuda() && v.device() == dev, fn, ": ", what, " must be on xq's GPU");
  TORCH_CHECK(v.scalar_type() == torch::kUInt8, fn, ": ", what, " must be uint8");
  TORCH_CHECK(v.is_contiguous(), fn, ": ", what, " must be contiguous");
  TORCH_CHECK(v.numel() == numel, fn, ": ", what, " must hold ", count, " bytes");
  TORCH_CHECK((uintptr_t)v.data_ptr() % align == 0, fn, ": ", what, " must be ", align,
              "-byte aligned");
}

// fused_mxfp4_gemm for any N >= 1 and any K >= 1 (llama_1b's gate/up: N = 5461,
// its down_proj: K = 5461); y has pitch N.  xq is [M, Kp128], Kp128 = K rounded
// up to 128, its pad columns zero codes: quantize_rows_fp8 for K % 128 == 0,
// quantize_rows_fp8_padded otherwise (the pad's contents are their contract,
// not checked here).  wq / wscales as quantize_rows_mxfp4 returns them for a
// [N,K] weight: N*Kp/2 and N*ceil(K/32) bytes, Kp = K rounded up to 32.  The
// ragged kernels load scale dwords from any byte address, so wscales may start
// anywhere; aligned N and K run the aligned kernel, which wants whole dwords.
torch::Tensor fused_mxfp4_gemm_ragged(torch::Tensor xq, torch::Tensor xs, torch::Tensor wq,
                                      torch::Tensor wscales, long N, long K, torch::Tensor t,
                                      torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_mxfp4_gemm_ragged";
  TORCH_CHECK(xq.is_cuda(), fn, ": xq must be a GPU tensor");
  TORCH_CHECK(xq.dim() == 2, fn, ": xq must be 2-D [M, Kp128]");
  const long M = xq.size(0);
  TORCH_CHECK(M > 0 && K > 0 && N > 0, fn, ": M, N and K must be > 0");
  TORCH_CHECK(M % 256 == 0, fn, " requires M%256==0");
  TORCH_CHECK(K < (1L << 24) && N < (1L << 31) && (M >> 8) * ((N + 255) >> 8) < (1L << 31), fn,
              ": shape too large");
  const long KA = (K + 127) / 128 * 128, bpr = (K + MX_BLOCK - 1) / MX_BLOCK;
  TORCH_CHECK(xq.size(1) == KA, fn, ": xq must have K rounded up to 128 columns");
  const bool krag = K % 128 != 0, nrag = N % 256 != 0;
  const auto dev = xq.device();
  check_mx_u8_ragged(fn, "x codes", xq, dev, M * KA, "M*Kp128", 16);
  TORCH_CHECK(xs.device() == dev, fn, ": x absmax must be on xq's device");
  TORCH_CHECK(xs.scalar_type() == torch::kFloat32, fn, ": x absmax must be fp32");
  TORCH_CHECK(xs.is_contiguous(), fn, ": x absmax must be contiguous");
  TORCH_CHECK(xs.numel() == M, fn, ": x absmax must hold one value per row");
  check_mx_u8_ragged(fn, "w codes", wq, dev, N * bpr * (MX_BLOCK / 2), "N*Kp/2", 16);
  check_mx_u8_ragged(fn, "w scales", wscales, dev, N * bpr, "N*ceil(K/32)",
                     krag || nrag ? 1 : 4);
  const LoraArgs a = prep_lora_bias(fn, "xq", dev, t, bw, bias, M, N, 64, 256, lora_scale);
  auto y = torch::empty({M, N}, xq.options().dtype(torch::kBFloat16));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((unsigned)((M >> 8) * ((N + 255) >> 8))), block(512);
#define LAUNCH_MX(RAG, KRAG)                                                                   \
  hipLaunchKernelGGL((fused_mxfp4_gemm_kernel<RAG, KRAG>), grid, block, MX_SMEM_BYTES, stream, \
                     xq.data_ptr<uint8_t>(), xs.data_ptr<float>(), wq.data_ptr<uint8_t>(),     \
                     (const unsigned*)wscales.data_ptr<uint8_t>(), a.t, a.bw, a.bias,          \
                     (__hip_bfloat16*)y.data_ptr(), M, N, K, a.r)
  if (krag) LAUNCH_MX(true, true);
  else if (nrag) LAUNCH_MX(true, false);
  else LAUNCH_MX(false, false);
#undef LAUNCH_MX
  HIP_CHECK_LAST();
  return y;
}

// ---------------------------------------------------------------------------
// fused_mxfp4_gemm_dx: dx = dy @ W from W's MXFP4 codes, on the fp8 cores.
//
// W's block scales run along k within a row n and dx reduces over n, so a
// scale is no factor of an output, cannot be folded into dy and is no block
// scale along the reduction.  Instead W is transcoded to e4m3 while it is
// staged, against one exponent per stripe (the 32 columns of an MX block
// column): E[kb] = max_n s[n,kb] comes from the host, and
//   B[n,k]  = e4m3_rne(e2m1(code[n,k]) * 2^(s[n,kb] - E[kb] + 6))
//   dx[m,k] = (sum_n g[m,n] B[n,k]) * (gs[m]/448) * 2^(E[kb] - 133)
// (ops/quant.py transcode_mxfp4_e4m3_ref is the definition).  B is exact up
// to a spread E - s of 14, |B| <= 384, no NaN code arises.
//
// Geometry of fused_fp8_gemm_dx (fp8_gemm.hip): 256x256 tile over [M,K], 8
// waves 2x4, XCD remap, 128-n reduction tiles, A = gq by glds into the swz_a
// image, double buffer, one vmcnt(0) + barrier per tile, the unscaled
// 16x16x128 f8f6f4 MFMA on two e4m3 operands (fragment chunks fq and 4+fq, the
// lane-to-k order the read-back tests found), a [256 k][128 n] byte B image
// under swz_a read by frag_e4m3, b128 row stores through LDS.
//
// The B stager.  A reduction tile of W is 128 rows x 128 bytes (256 k as
// nibbles, row pitch K/2).  A thread owns the 16 n x 4 k patch of fp8_gemm's
// dx kernel (k-quad q = l[1:0] | l[5:3]<<2 | w[0]<<5, n-chunk c = 2*w[2:1] +
// l[2]): 16 two-byte loads of codes and 16 one-byte loads of scales (4 k lie in
// one MX block: a byte per patch row, pitch K/32), issued one tile ahead right
// after A's glds and in flight during the 32 MFMAs.  A wave's code load covers
// 2 rows x 64 contiguous bytes.  (The 8 n x 8 k patch would load whole 128-byte
// rows, but its eight b64 writes of a 16-lane group fall on two swizzle values
// of one 8-byte column: 8-way.)  Behind the MFMAs each row's four nibbles go
// through v_cvt_scalef32_pk_f32_fp4 with the scale 2^(s - E + 6) (exact) and
// v_cvt_pk_fp8_f32 (the RNE, subnormals and signed zero of the definition):
// one dword W[n][4 k] of e4m3 bytes, 5 VALU a row.  From there on it is the
// fp8 patch: a byte transposition of four 4x4 blocks by v_perm_b32 and four
// b128 writes, conflict-free (tools/lds_bank_model.py mxfp4_dx_patch_writes).
// The stripe's E costs a thread one byte load for its patch and two for its
// accumulator columns (64 columns of a wave = 2 stripes).
// ---------------------------------------------------------------------------

#define MXDX_TILE_BYTES (256 * 128)
#define MXDX_BUF_A(b) (smem + (b) * (2 * MXDX_TILE_BYTES))
#define MXDX_BUF_B(b) (smem + (b) * (2 * MXDX_TILE_BYTES) + MXDX_TILE_BYTES)
#define MXDX_SMEM_BYTES (4 * MXDX_TILE_BYTES)  // 128 KiB

typedef __attribute__((ext_vector_type(2))) float f32x2_m;

// issue the loads of this thread's patch of one W reduction tile: `codes`
// points at the codes of W[n_tile0][k0], `scl` at the scale byte of that
// block (both uniform), `vo` / `so` are the lane's byte offsets
DEV_INLINE void load_w4_patch(unsigned (&st)[16], unsigned (&sc)[16], const char* codes,
                              const uint8_t* scl, long ldw, long bpr, unsigned vo, unsigned so) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    st[i] = *reinterpret_cast<const unsigned short*>(codes + (long)i * ldw + vo);
    sc[i] = scl[(long)i * bpr + so];
  }
}

// st[i]: four e2m1 codes W[n = 16c + i][k = 4q .. 4q+3] (low nibble first) ->
// their four e4m3 bytes at 2^(s - E + 6).  The spread E - s is clamped to
// 0..32: from 19 on every byte is a zero, and the scale stays a normal fp32.
DEV_INLINE void transcode_w4_patch(unsigned (&st)[16], const unsigned (&sc)[16], unsigned e) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int spread = min(max((int)e - (int)sc[i], 0), 32);
    const float f = __uint_as_float((unsigned)(133 - spread) << 23);
    const f32x2_m lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(st[i], f, 0);
    const f32x2_m hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(st[i], f, 1);
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(lo[0], lo[1], 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(hi[0], hi[1], p, true);
    st[i] = (unsigned)p;
  }
}

// st[i] holds B[n = 16c + i][k = 4q .. 4q+3]; write image rows 4q..4q+3,
// 16-byte chunk c (n = 16c .. 16c+15 ascending): fp8_gemm's write_b_patch
DEV_INLINE void write_bt_patch(char* image, const unsigned (&st)[16], int pq, int pc) {
  unsigned o[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const unsigned lo01 = __builtin_amdgcn_perm(st[4 * b + 1], st[4 * b + 0], 0x05010400u);
    const unsigned hi01 = __builtin_amdgcn_perm(st[4 * b + 1], st[4 * b + 0], 0x07030602u);
    const unsigned lo23 = __builtin_amdgcn_perm(st[4 * b + 3], st[4 * b + 2], 0x05010400u);
    const unsigned hi23 = __builtin_amdgcn_perm(st[4 * b + 3], st[4 * b + 2], 0x07030602u);
    o[0][b] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    o[1][b] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    o[2][b] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    o[3][b] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned p = swz_a((unsigned)(4 * pq + j) * 128u + (unsigned)pc * 16u);
    *reinterpret_cast<i32x4_m*>(image + p) =
        i32x4_m{(int)o[j][0], (int)o[j][1], (int)o[j][2], (int)o[j][3]};
  }
}

__global__ __launch_bounds__(512) void fused_mxfp4_gemm_dx_kernel(
    const uint8_t* __restrict__ gq,    // [M,N] e4m3 codes of dy
    const float* __restrict__ ga,      // [M] absmax of its rows
    const uint8_t* __restrict__ wq,    // [N,K/2] e2m1 codes of W
    const uint8_t* __restrict__ wsc,   // [N,K/32] E8M0 block scales
    const uint8_t* __restrict__ emax,  // [K/32] largest scale byte of each stripe
    __hip_bfloat16* __restrict__ dx,   // [M,K]
    long M, long N, long K) {
  // one __shared__ array only (glds pipeline rule)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][A | B] = 128 KiB

  // XCD-aware blockIdx remap (bijective form), as in fused_mxfp4_gemm_kernel
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbk = (int)(K >> 8);
  const long m0 = (long)(wgid / nbk) << 8;
  const long k0 = (long)(wgid % nbk) << 8;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 2;   // 0..1: wave m-position (128 rows)
  const int wc = wave & 3;    // 0..3: wave k-position (64 cols)
  const int fr = lane & 15;   // fragment row / C column
  const int fq = lane >> 4;   // fragment n-group / C row group

  // this thread's patch of every W tile
  const int pq = (lane & 3) | ((lane >> 3) << 2) | ((wave & 1) << 5);
  const int pc = (wave >> 1) * 2 + ((lane >> 2) & 1);
  const long ldw = K >> 1;  // code row pitch in bytes
  const long bpr = K >> 5;  // scale bytes per row
  // 32-bit lane offsets next to scalar row bases: 127 * K/2 + 126 < 2^30
  const unsigned voff = (unsigned)(pc * 16) * (unsigned)ldw + (unsigned)(pq * 2);
  const unsigned soff = (unsigned)(pc * 16) * (unsigned)bpr + (unsigned)(pq >> 3);
  const uint8_t* eb = emax + (k0 >> 5);   // the block's 8 stripes
  const unsigned ep = eb[pq >> 3];        // the patch's stripe

  f32x4_m acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_m{0.f, 0.f, 0.f, 0.f};

  const char* gg = (const char*)gq;
  const char* wg = (const char*)wq + (k0 >> 1);
  const uint8_t* sg8 = wsc + (k0 >> 5);
  const int NT = (int)(N >> 7);  // 128-n tiles
  unsigned st[16], sc[16];

  stage_a_tile(MXDX_BUF_A(0), gg, m0, N, 0, wave, lane);
  load_w4_patch(st, sc, wg, sg8, ldw, bpr, voff, soff);
  transcode_w4_patch(st, sc, ep);
  write_bt_patch(MXDX_BUF_B(0), st, pq, pc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int nt = 0; nt < NT; ++nt) {
    const int cur = nt & 1;
    const bool more = nt + 1 < NT;
    if (more) {
      stage_a_tile(MXDX_BUF_A(cur ^ 1), gg, m0, N, (long)(nt + 1) << 7, wave, lane);
      // keep the lane offsets opaque 32-bit VGPRs (saddr form): hoisted out
      // of the loop they become 32 64-bit lane addresses
      unsigned vo = voff, so = soff;
      asm volatile("" : "+v"(vo), "+v"(so));
      load_w4_patch(st, sc, wg + ((long)(nt + 1) << 7) * ldw, sg8 + ((long)(nt + 1) << 7) * bpr,
                    ldw, bpr, vo, so);
    }
    const char* A = MXDX_BUF_A(cur);
    const char* B = MXDX_BUF_B(cur);
    __builtin_amdgcn_s_setprio(1);
    // the 4 B fragments stay resident (32 VGPRs); A fragments stream through
    i32x8_m bf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = frag_e4m3(B, wc * 64 + j * 16 + fr, fq);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const i32x8_m af = frag_e4m3(A, wr * 128 + i * 16 + fr, fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            af, bf[j], acc[i][j], 0 /*A e4m3*/, 0 /*B e4m3*/, 0, 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    // the other B image was last read in the previous iteration, behind its
    // barrier; the patch loads had the whole MFMA loop to land
    if (more) {
      transcode_w4_patch(st, sc, ep);
      write_bt_patch(MXDX_BUF_B(cur ^ 1), st, pq, pc);
    }
    // drain next tile's glds, then release the buffers we just read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- gs[m]/448, then the stripe's power of two applied exactly (ldexp);
  // a wave's 64 columns are two stripes, column fragments 0-1 and 2-3
  const int e2[2] = {(int)eb[wc * 2] - 133, (int)eb[wc * 2 + 1] - 133};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4_m ax = *reinterpret_cast<const f32x4_m*>(ga + m0 + wr * 128 + i * 16 + fq * 4);
    const f32x4_m sg = {__fdiv_rn(ax[0], E4M3_MAX), __fdiv_rn(ax[1], E4M3_MAX),
                        __fdiv_rn(ax[2], E4M3_MAX), __fdiv_rn(ax[3], E4M3_MAX)};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        acc[i][j][reg] = ldexpf(__fmul_rn(acc[i][j][reg], sg[reg]), e2[j >> 1]);
  }
  // ---- one bf16 rounding, b128 row stores through LDS (16 KiB per wave)
  __bf16* mine = (__bf16*)smem + wave * (128 * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        mine[(i * 16 + fq * 4 + reg) * 64 + j * 16 + fr] = (__bf16)acc[i][j][reg];
  // no barrier needed: each wave reads only its own region
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (lane >> 3);          // 0..127
    const int cb = (lane & 7) * 8;                 // 8-col chunk
    const bf16x8_m vv = *reinterpret_cast<const bf16x8_m*>(mine + row * 64 + cb);
    *reinterpret_cast<bf16x8_m*>(dx + (m0 + wr * 128 + row) * K + k0 + wc * 64 + cb) = vv;
  }
}

// one uint8 operand of fused_mxfp4_gemm_dx; `align` 1 for none
static void check_mx_dx_u8(const char* fn, const char* what, const torch::Tensor& v,
                           const torch::Device& dev, long numel, const char* count, int align) {
  TORCH_CHECK(v.is_cuda() && v.device() == dev, fn, ": ", what, " must be on gq's GPU");
  TORCH_CHECK(v.scalar_type() == torch::kUInt8, fn, ": ", what, " must be uint8");
  TORCH_CHECK(v.is_contiguous(), fn, ": ", what, " must be contiguous");
  TORCH_CHECK(v.numel() == numel, fn, ": ", what, " must hold ", count, " bytes");
  TORCH_CHECK((uintptr_t)v.data_ptr() % align == 0, fn, ": ", what, " must be ", align,
              "-byte aligned");
}

// gq / gs: quantize_rows_fp8(dy) [M,N]; wq / wscales as stored for a [N,K]
// weight; emax [K/32]: the column maximum of wscales.  The kernel indexes from
// M, N and K alone, so every size is checked against them here.
torch::Tensor fused_mxfp4_gemm_dx(torch::Tensor gq, torch::Tensor gs, torch::Tensor wq,
                                  torch::Tensor wscales, torch::Tensor emax, long N, long K) {
  const char* fn = "fused_mxfp4_gemm_dx";
  TORCH_CHECK(gq.is_cuda(), fn, ": gq must be a GPU tensor");
  TORCH_CHECK(gq.dim() == 2, fn, ": gq must be 2-D [M, N]");
  const long M = gq.size(0);
  TORCH_CHECK(M > 0 && N > 0 && K > 0, fn, ": M, N and K must be > 0");
  TORCH_CHECK(M % 256 == 0 && K % 256 == 0 && N % 128 == 0, fn,
              " requires M%256==0, K%256==0, N%128==0");
  TORCH_CHECK(K < (1L << 24) && N < (1L << 31) && (M >> 8) * (K >> 8) < (1L << 31), fn,
              ": shape too large");
  const auto dev = gq.device();
  check_mx_dx_u8(fn, "g codes", gq, dev, M * N, "M*N", 16);
  TORCH_CHECK(gs.device() == dev, fn, ": g absmax must be on gq's device");
  TORCH_CHECK(gs.scalar_type() == torch::kFloat32, fn, ": g absmax must be fp32");
  TORCH_CHECK(gs.is_contiguous(), fn, ": g absmax must be contiguous");
  TORCH_CHECK(gs.dim() == 1 && gs.numel() == M, fn, ": g absmax must hold one value per row");
  check_mx_dx_u8(fn, "w codes", wq, dev, N * K / 2, "N*K/2", 16);
  check_mx_dx_u8(fn, "w scales", wscales, dev, N * K / MX_BLOCK, "N*K/32", 1);
  check_mx_dx_u8(fn, "stripe exponents", emax, dev, K / MX_BLOCK, "K/32", 1);
  auto dx = torch::empty({M, K}, gq.options().dtype(torch::kBFloat16));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((unsigned)((M >> 8) * (K >> 8))), block(512);
  hipLaunchKernelGGL(fused_mxfp4_gemm_dx_kernel, grid, block, MXDX_SMEM_BYTES, stream,
                     gq.data_ptr<uint8_t>(), gs.data_ptr<float>(), wq.data_ptr<uint8_t>(),
                     wscales.data_ptr<uint8_t>(), emax.data_ptr<uint8_t>(),
                     (__hip_bfloat16*)dx.data_ptr(), M, N, K);
  HIP_CHECK_LAST();
  return dx;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
