// Some packed-fp32 instruction forms miscompute on this target, so this file
// is compiled without them.  The attribute has to cover the headers too: a
// helper that lacks it is not inlined into a function that has it.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "hip/hip_runtime.h"
// FP8 frozen-W path (`--quantize fp8`) on the gfx950 f8f6f4 matrix cores.
//
// Format: OCP e4m3 (e4m3fn, max 448), ONE fp32 absmax per row, no block
// scales.  For a row v:  inv = 448/absmax (one IEEE fp32 division),
// code = e4m3_rne(v*inv) with the product rounded to fp32,
// value = float(code) * (absmax/448).  A row of zeros encodes to zeros.
// W [N,K] is quantised per output row (once per merge cycle), activations
// [M,K] per token row at every forward.  Both scales are rank-1 over the
// output, so the MFMA loop runs on raw codes and the scales enter in the
// epilogue only:  y[m,n] = acc[m,n] * (ax[m]/448) * (aw[n]/448).
//
//   quantize_rows_fp8    bf16 [R,K] -> (uint8 codes [R,K], fp32 absmax [R])
//   dequantize_rows_fp8  codes, absmax -> bf16 | fp32 [R,K]
//   fused_fp8_gemm       y = (xq·wq^T)·sx·sw^T (+bias) + s·t·Bw^T, bf16 out
//   ..._ragged / _padded any N (out_features);  ..._kragged / quantize_rows_fp8_padded
//                        any K (in_features) as well: W's rows through registers
//
// GEMM structure: the 256x256 / 8-wave / double-buffered-glds geometry of
// fused_lora_gemm, redesigned for one-byte operands.  An LDS row stays
// 128 bytes — now 128 k — so a K-tile carries twice the k of the bf16 kernel
// for the same bytes, the same glds count and the same barrier count, and one
// v_mfma_f32_16x16x128_f8f6f4 per C fragment consumes the whole tile row.
//
// Tile instruction: 16x16x128 rather than 32x32x64.  Per 128 k a wave's
// 128x64 tile needs 12 32-byte fragments either way, so LDS traffic is the
// same; 16x16x128 keeps the 16x16 C layout (col = lane&15, row =
// (lane>>4)*4+reg), so the rank-r LoRA update lands on the SAME accumulators
// with the 16x16x32 bf16 MFMAs and the LDS-staged b128 store epilogue of
// fused_lora_gemm carries over unchanged.
//
// Lane-to-k assignment: a dot product is invariant under any permutation of
// k that A and B share, so lane (row fr = lane&15, group fq = lane>>4) takes
// its 32 bytes as the two 16-byte chunks {fq, 4+fq} of the row (k =
// fq*16..+16 and 64+fq*16..+16) rather than 32 consecutive k.  With the
// swizzle  chunk ^= (row>>1)&7  every 16-lane ds_read_b128 service group
// covers all 16 16-byte bank slots exactly once: conflict-free for both
// reads of the fp8 fragments and for the bf16 LoRA fragments (chunk
// ks*4+fq), checked with tools/lds_bank_model.py (fp8_gemm_* patterns).

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"
#include "gemm_host.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_q;
typedef __attribute__((ext_vector_type(4))) float f32x4_q;
typedef __attribute__((ext_vector_type(4))) int i32x4_q;
typedef __attribute__((ext_vector_type(8))) int i32x8_q;

#define FP8_MAX 448.0f

// ---------------------------------------------------------------------------
// Row quantiser.  One pass over HBM: a row sits on G lanes (a wave, or 16
// lanes for K <= 256), each lane keeps NU units of 16 bf16 (two bf16x8 loads)
// in registers between the shuffle max-reduction and the packed conversion,
// and stores 16 codes per unit with one 16-byte store.  NU == 0 is the
// looping form for K > 8192 (second read of the row comes from L2).
// ---------------------------------------------------------------------------

struct Unit16 { uint4 lo, hi; };  // 16 bf16

DEV_INLINE float unit_absmax(const Unit16& u) {
  const unsigned w[8] = {u.lo.x, u.lo.y, u.lo.z, u.lo.w, u.hi.x, u.hi.y, u.hi.z, u.hi.w};
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    am = fmaxf(am, fabsf(__uint_as_float(w[i] << 16)));
    am = fmaxf(am, fabsf(__uint_as_float(w[i] & 0xffff0000u)));
  }
  return am;
}

DEV_INLINE uint4 unit_encode(const Unit16& u, float inv) {
  const unsigned w[8] = {u.lo.x, u.lo.y, u.lo.z, u.lo.w, u.hi.x, u.hi.y, u.hi.z, u.hi.w};
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = __fmul_rn(__uint_as_float(w[2 * i] << 16), inv);
    const float b = __fmul_rn(__uint_as_float(w[2 * i] & 0xffff0000u), inv);
    const float c = __fmul_rn(__uint_as_float(w[2 * i + 1] << 16), inv);
    const float d = __fmul_rn(__uint_as_float(w[2 * i + 1] & 0xffff0000u), inv);
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
    o[i] = (unsigned)p;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

template <int G>
DEV_INLINE float group_max(float am) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) am = fmaxf(am, __shfl_xor(am, off));
  return am;
}

// Unit c of a row of any length K, for the padded form: units wholly below K
// load two Vec8 (rows of odd K are only 2-byte aligned), the unit that
// straddles K loads element by element behind a guard, units at or past K are
// zeros.
DEV_INLINE Unit16 unit_load_ragged(const __hip_bfloat16* __restrict__ xrow, int c, int K) {
  Unit16 u;
  if (c * 16 + 16 <= K) {
    const Vec8<__hip_bfloat16> a = load8(xrow + c * 16), b = load8(xrow + c * 16 + 8);
    __builtin_memcpy(&u.lo, &a, 16);
    __builtin_memcpy(&u.hi, &b, 16);
  } else {
    const unsigned short* bits = reinterpret_cast<const unsigned short*>(xrow);
    unsigned w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = c * 16 + 2 * i;
      const unsigned lo = k < K ? bits[k] : 0u, hi = k + 1 < K ? bits[k + 1] : 0u;
      w[i] = lo | (hi << 16);
    }
    u.lo = make_uint4(w[0], w[1], w[2], w[3]);
    u.hi = make_uint4(w[4], w[5], w[6], w[7]);
  }
  return u;
}

// PAD: any K >= 1; the code rows have pitch Kp = K rounded up to 128 and the
// bytes [K, Kp) are zero codes, so the rows are 16-byte aligned glds sources
// and whole 128-k tiles for fused_fp8_gemm_kernel<true, true>.
template <int G, int NU, bool PAD>
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(
    const __hip_bfloat16* __restrict__ x, uint8_t* __restrict__ q,
    float* __restrict__ absmax, long R, int K) {
  const int gl = threadIdx.x & (G - 1);
  const long row = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  const bool live = row < R;  // whole lane groups: shuffles stay inside a row
  const int Kp = PAD ? (K + 127) & ~127 : K;
  const int units = Kp >> 4;
  const __hip_bfloat16* xrow = x + (live ? row : 0) * K;
  const Unit16* src = reinterpret_cast<const Unit16*>(x + (live ? row : 0) * K);
  uint4* dst = reinterpret_cast<uint4*>(q + (live ? row : 0) * Kp);
  float am = 0.f;
  if (NU > 0) {
    Unit16 u[NU > 0 ? NU : 1];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int c = gl + i * G;
      if (PAD)
        u[i] = (live && c < units) ? unit_load_ragged(xrow, c, K)
                                   : Unit16{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
      else
        u[i] = (live && c < units) ? src[c] : Unit16{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
      am = fmaxf(am, unit_absmax(u[i]));
    }
    am = group_max<G>(am);
    const float inv = am > 0.f ? __fdiv_rn(FP8_MAX, am) : 0.f;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int c = gl + i * G;
      if (live && c < units) dst[c] = unit_encode(u[i], inv);
    }
  } else {
    if (live)
      for (int c = gl; c < units; c += G)
        am = fmaxf(am, unit_absmax(PAD ? unit_load_ragged(xrow, c, K) : src[c]));
    am = group_max<G>(am);
    const float inv = am > 0.f ? __fdiv_rn(FP8_MAX, am) : 0.f;
    if (live)
      for (int c = gl; c < units; c += G)
        dst[c] = unit_encode(PAD ? unit_load_ragged(xrow, c, K) : src[c], inv);
  }
  if (live && gl == 0) absmax[row] = am;
}

// any K (weights whose in_features is no multiple of 16, e.g. 5461): one wave
// per row, scalar loads, byte stores.  Off the hot path (once per merge).
__global__ __launch_bounds__(256) void quantize_rows_fp8_any_kernel(
    const __hip_bfloat16* __restrict__ x, uint8_t* __restrict__ q,
    float* __restrict__ absmax, long R, int K) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = row < R;
  const __hip_bfloat16* src = x + (live ? row : 0) * K;
  float am = 0.f;
  if (live)
    for (int k = lane; k < K; k += 64) am = fmaxf(am, fabsf(to_f32(src[k])));
  am = group_max<64>(am);
  if (!live) return;
  const float inv = am > 0.f ? __fdiv_rn(FP8_MAX, am) : 0.f;
  for (int k = lane; k < K; k += 64) {
    const int p = __builtin_amdgcn_cvt_pk_fp8_f32(__fmul_rn(to_f32(src[k]), inv), 0.f, 0, false);
    q[row * K + k] = (uint8_t)(p & 0xff);
  }
  if (lane == 0) absmax[row] = am;
}

template <int G, int NU, bool PAD = false>
static void launch_quantize(const torch::Tensor& x, torch::Tensor& q, torch::Tensor& am,
                            long R, int K, hipStream_t stream) {
  const long rows_per_block = 256 / G;
  dim3 grid((unsigned)((R + rows_per_block - 1) / rows_per_block)), block(256);
  hipLaunchKernelGGL((quantize_rows_fp8_kernel<G, NU, PAD>), grid, block, 0, stream,
                     (const __hip_bfloat16*)x.data_ptr(), q.data_ptr<uint8_t>(),
                     am.data_ptr<float>(), R, K);
}

template <bool PAD>
static std::vector<torch::Tensor> quantize_rows_fp8_impl(const char* fn, torch::Tensor x) {
  TORCH_CHECK(x.is_cuda(), fn, ": x must be a GPU tensor");
  TORCH_CHECK(x.dim() == 2, fn, ": x must be 2-D [R, K]");
  TORCH_CHECK(x.is_contiguous(), fn, ": x must be contiguous");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, fn, ": x must be bf16");
  const long R = x.size(0), K = x.size(1);
  TORCH_CHECK(R > 0 && K > 0, fn, ": R and K must be > 0");
  TORCH_CHECK(K < (1L << 31) - (PAD ? 128 : 0) && R < (1L << 31) * 4, fn, ": shape too large");
  const long Kp = PAD ? (K + 127) / 128 * 128 : K;  // the form is chosen by the padded width
  auto q = torch::empty({R, Kp}, x.options().dtype(torch::kUInt8));
  auto am = torch::empty({R}, x.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int k = (int)K;
  if (!PAD && K % 16 != 0) {
    hipLaunchKernelGGL(quantize_rows_fp8_any_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256),
                       0, stream, (const __hip_bfloat16*)x.data_ptr(), q.data_ptr<uint8_t>(),
                       am.data_ptr<float>(), R, k);
  } else if (Kp <= 256) {
    launch_quantize<16, 1, PAD>(x, q, am, R, k, stream);
  } else if (Kp <= 1024) {
    launch_quantize<64, 1, PAD>(x, q, am, R, k, stream);
  } else if (Kp <= 2048) {
    launch_quantize<64, 2, PAD>(x, q, am, R, k, stream);
  } else if (Kp <= 4096) {
    launch_quantize<64, 4, PAD>(x, q, am, R, k, stream);
  } else if (Kp <= 8192) {
    launch_quantize<64, 8, PAD>(x, q, am, R, k, stream);
  } else {
    launch_quantize<64, 0, PAD>(x, q, am, R, k, stream);
  }
  HIP_CHECK_LAST();
  return {q, am};
}

std::vector<torch::Tensor> quantize_rows_fp8(torch::Tensor x) {
  return quantize_rows_fp8_impl<false>("quantize_rows_fp8", x);
}

// any K >= 1: codes [R, Kp], Kp = K rounded up to 128, the pad bytes zero codes
std::vector<torch::Tensor> quantize_rows_fp8_padded(torch::Tensor x) {
  return quantize_rows_fp8_impl<true>("quantize_rows_fp8_padded", x);
}

// ---------------------------------------------------------------------------
// Row dequantiser: value = float(code) * (absmax/448), rounded once to T.
// VEC: one thread per 16 codes (K % 16 == 0); otherwise one per code.
// ---------------------------------------------------------------------------

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dequantize_rows_fp8_kernel(
    const uint8_t* __restrict__ q, const float* __restrict__ absmax,
    T* __restrict__ out, long n, int K) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * (VEC ? 16 : 1);
  if (i >= n) return;
  const float sc = __fdiv_rn(absmax[i / K], FP8_MAX);
  if (VEC) {
    const uint4 c = *reinterpret_cast<const uint4*>(q + i);
    const unsigned w[4] = {c.x, c.y, c.z, c.w};
    T v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[4 * j + 0] = from_f32<T>(__fmul_rn(__builtin_amdgcn_cvt_f32_fp8(w[j], 0), sc));
      v[4 * j + 1] = from_f32<T>(__fmul_rn(__builtin_amdgcn_cvt_f32_fp8(w[j], 1), sc));
      v[4 * j + 2] = from_f32<T>(__fmul_rn(__builtin_amdgcn_cvt_f32_fp8(w[j], 2), sc));
      v[4 * j + 3] = from_f32<T>(__fmul_rn(__builtin_amdgcn_cvt_f32_fp8(w[j], 3), sc));
    }
    store8(out + i, *reinterpret_cast<const Vec8<T>*>(v));
    store8(out + i + 8, *reinterpret_cast<const Vec8<T>*>(v + 8));
  } else {
    out[i] = from_f32<T>(__fmul_rn(__builtin_amdgcn_cvt_f32_fp8((unsigned)q[i], 0), sc));
  }
}

torch::Tensor dequantize_rows_fp8(torch::Tensor q, torch::Tensor absmax, long R, long K,
                                  torch::ScalarType dtype) {
  const char* fn = "dequantize_rows_fp8";
  TORCH_CHECK(q.is_cuda(), fn, ": codes must be a GPU tensor");
  TORCH_CHECK(q.scalar_type() == torch::kUInt8 && q.is_contiguous(), fn,
              ": codes must be contiguous uint8");
  TORCH_CHECK(R > 0 && K > 0 && K < (1L << 31), fn, ": bad R or K");
  TORCH_CHECK(q.numel() == R * K, fn, ": codes must hold R*K values");
  TORCH_CHECK(absmax.device() == q.device() && absmax.scalar_type() == torch::kFloat32 &&
                  absmax.is_contiguous() && absmax.numel() == R,
              fn, ": absmax must be R contiguous fp32 values on the codes' device");
  TORCH_CHECK(dtype == torch::kBFloat16 || dtype == torch::kFloat32, fn,
              ": output dtype must be bf16 or fp32");
  auto out = torch::empty({R, K}, q.options().dtype(dtype));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const long n = R * K;
  const bool vec = K % 16 == 0;
  const long threads = vec ? n / 16 : n;
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  const uint8_t* qp = q.data_ptr<uint8_t>();
  const float* ap = absmax.data_ptr<float>();
#define LAUNCH_DQ(T, PTR, V)                                                          \
  hipLaunchKernelGGL((dequantize_rows_fp8_kernel<T, V>), grid, block, 0, stream, qp,  \
                     ap, PTR, n, (int)K)
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
// fused_fp8_gemm
// ---------------------------------------------------------------------------

// Swizzle on a byte offset within a [rows][128 B] image: the 16-byte chunk
// index (bits 4..6) ^= (row>>1)&7 (bits 8..10).  An involution that keeps the
// row, so the same function maps LDS byte -> source byte when staging and
// logical byte -> LDS byte when reading.
DEV_INLINE unsigned swz8(unsigned o) { return o ^ (((o >> 8) & 7u) << 4); }

// Stage one [256][128 B] tile (32 KiB) into `image` via glds: 32 wave-level
// 1-KiB pieces (8 full rows each), 4 per wave.  The LDS image is lane-linear
// as glds requires; the per-lane GLOBAL source address carries the swizzle.
// `gbase` is a byte pointer, `ld` the row pitch in bytes, `k0` a byte offset.
// CLAMP: rows past `last` read row `last` instead (the edge tile of a ragged
// operand: nothing outside the allocation is touched, the image rows hold
// garbage that only feeds accumulators nobody stores).
template <bool CLAMP = false>
DEV_INLINE void stage_tile_bytes(char* image, const char* gbase, long row0, long ld,
                                 long k0, int wave, int lane, long last = 0) {
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) {
    const int piece = wave * 4 + p4;
    const unsigned s = swz8(piece * 1024u + lane * 16u);  // source byte in tile
    long row = row0 + (s >> 7);
    if (CLAMP) row = row < last ? row : last;
    const char* src = gbase + row * ld + k0 + (s & 127u);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// fp8 A/B fragment of the 16x16x128 MFMA: chunks fq and 4+fq of `row`
DEV_INLINE i32x8_q frag_fp8(const char* image, int row, int fq) {
  const unsigned p = swz8((unsigned)row * 128u + (unsigned)fq * 16u);
  const i32x4_q lo = *reinterpret_cast<const i32x4_q*>(image + p);
  const i32x4_q hi = *reinterpret_cast<const i32x4_q*>(image + (p ^ 64u));
  return i32x8_q{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// bf16 fragment (16x16x32 layout: lane -> row l&15, 8 k at ks*32 + (l>>4)*8)
DEV_INLINE bf16x8_q frag_bf16(const char* image, int row, int ks, int fq) {
  const unsigned o = (unsigned)row * 128u + (unsigned)ks * 64u + (unsigned)fq * 16u;
  return *reinterpret_cast<const bf16x8_q*>(image + swz8(o));
}

#define FP8_TILE_BYTES (256 * 128)
#define FP8_BUF_A(b) (smem + (b) * (2 * FP8_TILE_BYTES))
#define FP8_BUF_B(b) (smem + (b) * (2 * FP8_TILE_BYTES) + FP8_TILE_BYTES)

// --- register-staged B operand for a ragged reduction width (KRAG) ----------
// W's code rows have pitch K, any K >= 1: a row starts at any byte alignment,
// which glds cannot source.  Each thread owns four 16-byte chunks of the
// [256][128 B] tile: chunk c = lane&7 of rows rt + 8i, rt = wave*32 + (lane>>3).
// A wave's load instruction covers 8 whole rows of 128 contiguous bytes with
// unaligned 16-byte loads (one global_load_dwordx4 each); an 8-lane
// ds_write_b128 group holds the 8 chunks of one row, which swz8 permutes
// within the row's 128 bytes: conflict-free (tools/lds_bank_model.py
// fp8_kragged_b_writes).

DEV_INLINE i32x4_q load16_any(const char* p) {
  i32x4_q v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// rows past `nrel` (the last row of W, relative to the tile) read row nrel;
// `cb` is the lane's byte offset within a row, relative to `base`
DEV_INLINE void load_b_rows(i32x4_q (&st)[4], const char* base, unsigned K, int rt, int nrel,
                            unsigned cb) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = rt + 8 * i < nrel ? rt + 8 * i : nrel;
    st[i] = load16_any(base + ((unsigned)row * K + cb));
  }
}

// K < 16: a row is shorter than one chunk; bytes behind a guard, chunk 0 only
DEV_INLINE void load_b_rows_bytes(i32x4_q (&st)[4], const char* base, unsigned K, int rt,
                                  int nrel, int c) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = rt + 8 * i < nrel ? rt + 8 * i : nrel;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    if (c == 0) {
#pragma unroll
      for (unsigned e = 0; e < 15; ++e)
        if (e < K) w[e >> 2] |= (unsigned)(uint8_t)base[(unsigned)row * K + e] << (8 * (e & 3));
    }
    st[i] = i32x4_q{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
  }
}

// v >> 8*s over the 16 bytes, zeros shifted in; s is wave-uniform, 1..15
DEV_INLINE i32x4_q shr_bytes(const i32x4_q& v, int s) {
  const unsigned w[8] = {(unsigned)v[0], (unsigned)v[1], (unsigned)v[2], (unsigned)v[3], 0u, 0u, 0u, 0u};
  const int sd = s >> 2;
  const unsigned sb = (unsigned)s & 3u;
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned lo = sd == 0 ? w[i] : sd == 1 ? w[i + 1] : sd == 2 ? w[i + 2] : w[i + 3];
    const unsigned hi = sd == 0 ? w[i + 1] : sd == 1 ? w[i + 2] : sd == 2 ? w[i + 3] : w[i + 4];
    o[i] = __builtin_amdgcn_alignbyte(hi, lo, sb);
  }
  return i32x4_q{(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
}

// The last tile holds kv < 128 valid bytes a row.  Chunks wholly below kv load
// as usual.  The chunk that straddles kv was loaded END-aligned (the 16 bytes
// that end with the row, so nothing behind the row is read — for the last row
// that would be outside wq) and is shifted down here; chunks at or past kv are
// cleared.  Zeros, not A's zero pad, keep the bytes at k >= K out of the sums:
// 0x7F/0xFF are NaN in e4m3 and 0 x NaN is NaN.
DEV_INLINE void fix_b_rows_edge(i32x4_q (&st)[4], int c, int kv) {
  const int cs = kv >> 4, rem = kv & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const i32x4_q sh = shr_bytes(st[i], (16 - rem) & 15);
    const i32x4_q z = {0, 0, 0, 0};
    st[i] = c < cs ? st[i] : (c == cs && rem != 0) ? sh : z;
  }
}

DEV_INLINE void write_b_rows(char* image, const i32x4_q (&st)[4], int rt, int c) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<i32x4_q*>(image + swz8((unsigned)(rt + 8 * i) * 128u + (unsigned)c * 16u)) =
        st[i];
}

// RAGGED: any N >= 1.  The grid has ceil(N/256) block columns; in the last one
// every W-side row index >= N (B tile, bw tile, wa, bias) is clamped to N-1,
// and the epilogue stores rows of pitch N up to column N only.
// KRAG (with RAGGED): any K >= 1 as well.  xq has pitch Kp = K rounded up to
// 128 with zero codes in [K, Kp) (quantize_rows_fp8_padded) and comes by glds
// as before; wq has pitch K and comes through registers (above), fetched one
// tile ahead right after A's glds is issued, in flight during the MFMAs and
// written to the other B image behind them.
template <bool RAGGED, bool KRAG = false>
__global__ __launch_bounds__(512) void fused_fp8_gemm_kernel(
    const uint8_t* __restrict__ xq,         // [M,K] e4m3 codes
    const float* __restrict__ xa,           // [M] absmax of x rows
    const uint8_t* __restrict__ wq,         // [N,K] e4m3 codes
    const float* __restrict__ wa,           // [N] absmax of W rows
    const __hip_bfloat16* __restrict__ t,   // [M,r] or null (pre-scaled)
    const __hip_bfloat16* __restrict__ bw,  // [N,r] or null
    const __hip_bfloat16* __restrict__ bias,  // [N] or null
    __hip_bfloat16* __restrict__ y,         // [M,N]
    long M, long N, long K, int r) {
  // one __shared__ array only (glds pipeline rule)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][A | B] = 128 KiB

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
  const int fq = lane >> 4;   // fragment k-group / C row group

  f32x4_q acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_q{0.f, 0.f, 0.f, 0.f};

  // buffer b: A image at smem + b*64 KiB, B image 32 KiB behind it
  const char* xg = (const char*)xq;
  const char* wg = (const char*)wq;

  const long KA = KRAG ? (K + 127) & ~127L : K;  // pitch of xq, reduction depth
  const int KT = (int)(KA >> 7);                 // 128-k tiles
  // KRAG: this thread's chunks of every B tile, W's rows relative to row n0,
  // valid bytes a row in the last tile
  const int rt = wave * 32 + (lane >> 3), bc = lane & 7;
  const int nrel = (int)(nl - n0 < 255 ? nl - n0 : 255);
  const int kv = (int)(K - ((long)(KT - 1) << 7));
  const char* wrow = wg + n0 * K;
  i32x4_q st[4];
  stage_tile_bytes(FP8_BUF_A(0), xg, m0, KA, 0, wave, lane);
  if (KRAG) {
    if (K < 16) {
      load_b_rows_bytes(st, wrow, (unsigned)K, rt, nrel, bc);
    } else if (KT == 1 && kv < 128) {
      load_b_rows(st, wrow, (unsigned)K, rt, nrel,
                  bc < (kv >> 4) ? (unsigned)bc * 16u : (unsigned)K - 16u);
      fix_b_rows_edge(st, bc, kv);
    } else {
      load_b_rows(st, wrow, (unsigned)K, rt, nrel, (unsigned)bc * 16u);
    }
    write_b_rows(FP8_BUF_B(0), st, rt, bc);
  } else {
    stage_tile_bytes<RAGGED>(FP8_BUF_B(0), wg, n0, K, 0, wave, lane, nl);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < KT;
    const bool edge = KRAG && kt + 2 == KT && kv < 128;  // uniform: next tile is short
    if (more) {
      stage_tile_bytes(FP8_BUF_A(cur ^ 1), xg, m0, KA, (long)(kt + 1) << 7, wave, lane);
      if (KRAG) {
        // the lane's row and chunk stay opaque 32-bit VGPRs next to a scalar
        // base (saddr form): hoisted out of the loop the four offsets become
        // 64-bit lane addresses
        int ro = rt;
        unsigned co = (unsigned)bc * 16u;
        asm volatile("" : "+v"(ro), "+v"(co));
        const unsigned k0 = (unsigned)(kt + 1) << 7;
        if (edge) {  // K >= 128 here; full chunks as usual, the others end-aligned
          load_b_rows(st, wrow, (unsigned)K, ro, nrel,
                      bc < (kv >> 4) ? k0 + co : (unsigned)K - 16u);
        } else {
          load_b_rows(st, wrow + k0, (unsigned)K, ro, nrel, co);
        }
      } else {
        stage_tile_bytes<RAGGED>(FP8_BUF_B(cur ^ 1), wg, n0, K, (long)(kt + 1) << 7, wave, lane,
                                 nl);
      }
    }
    const char* A = FP8_BUF_A(cur);
    const char* B = FP8_BUF_B(cur);
    __builtin_amdgcn_s_setprio(1);
    // the 4 B fragments stay resident (32 VGPRs); A fragments stream through
    i32x8_q bf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = frag_fp8(B, wc * 64 + j * 16 + fr, fq);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const i32x8_q af = frag_fp8(A, wr * 128 + i * 16 + fr, fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            af, bf[j], acc[i][j], 0 /*A e4m3*/, 0 /*B e4m3*/, 0, 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    if (KRAG) {
      // the other B image was last read in the previous iteration, behind its
      // barrier; the chunk loads had the whole MFMA loop to land
      if (edge) fix_b_rows_edge(st, bc, kv);
      if (more) write_b_rows(FP8_BUF_B(cur ^ 1), st, rt, bc);
    }
    // drain next tile's glds, then release the buffers we just read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- 1. rank-1 scales on the resident accumulators (fp32) --------------
  {
    float sw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long n = n0 + wc * 64 + j * 16 + fr;
      if (RAGGED) n = n < nl ? n : nl;
      sw[j] = __fdiv_rn(wa[n], FP8_MAX);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4_q ax =
          *reinterpret_cast<const f32x4_q*>(xa + m0 + wr * 128 + i * 16 + fq * 4);
      const f32x4_q sx = {__fdiv_rn(ax[0], FP8_MAX), __fdiv_rn(ax[1], FP8_MAX),
                          __fdiv_rn(ax[2], FP8_MAX), __fdiv_rn(ax[3], FP8_MAX)};
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] * (sx * sw[j]);
    }
  }

  // ---- 2. LoRA rank-r update: acc += t_s-tile @ Bw-tile^T (bf16 MFMA) -----
  if (r > 0) {
    const int RC = r >> 6;  // [256][64] bf16 chunks per operand
    const long ldr = (long)r * 2;
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_tile_bytes(FP8_BUF_A(c & 1), (const char*)t, m0, ldr, (long)c << 7, wave, lane);
      stage_tile_bytes<RAGGED>(FP8_BUF_B(c & 1), (const char*)bw, n0, ldr, (long)c << 7, wave,
                               lane, nl);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const char* A = FP8_BUF_A(c & 1);
      const char* B = FP8_BUF_B(c & 1);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_q bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = frag_bf16(B, wc * 64 + j * 16 + fr, ks, fq);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bf16x8_q afr = frag_bf16(A, wr * 128 + i * 16 + fr, ks, fq);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[j], acc[i][j],
                                                                0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();
    }
  }

  // ---- 3+4. bias, one bf16 rounding, b128 row stores through LDS ----------
  __syncthreads();
  __bf16* mine = (__bf16*)smem + wave * (128 * 64);  // 16 KiB per wave
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + fq * 4 + reg;  // within wave tile
        const int col = j * 16 + fr;
        float v = acc[i][j][reg];
        if (bias) {
          long n = n0 + wc * 64 + col;
          if (RAGGED) n = n < nl ? n : nl;
          v += (float)bias[n];
        }
        mine[row * 64 + col] = (__bf16)v;
      }
  // no barrier needed: each wave reads only its own region
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (lane >> 3);          // 0..127
    const int cb = (lane & 7) * 8;                 // 8-col chunk
    const bf16x8_q vv = *reinterpret_cast<const bf16x8_q*>(mine + row * 64 + cb);
    if (RAGGED) {
      // pitch N: with N % 8 != 0 a row start is only 2-byte aligned, so the
      // 16-byte store goes through Vec8 (alignof 2), as in norms.hip; the
      // chunk that straddles N goes element by element, later ones are skipped
      const long col = n0 + wc * 64 + cb;
      __hip_bfloat16* dst = y + (m0 + wr * 128 + row) * N + col;
      if (col + 8 <= N) {
        store8(dst, *reinterpret_cast<const Vec8<__hip_bfloat16>*>(&vv));
      } else {
        const __hip_bfloat16* sv = reinterpret_cast<const __hip_bfloat16*>(&vv);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < N) dst[e] = sv[e];
      }
    } else {
      *reinterpret_cast<bf16x8_q*>(y + (m0 + wr * 128 + row) * N + n0 + wc * 64 + cb) = vv;
    }
  }
}

// codes [rows*k] uint8 and absmax [rows] fp32, both contiguous, on x's device
static void check_fp8_operand(const char* fn, const char* what, const torch::Tensor& q,
                              const torch::Tensor& a, const torch::Device& dev, long rows,
                              long k) {
  TORCH_CHECK(q.is_cuda() && q.device() == dev, fn, ": ", what, " codes must be on xq's GPU");
  TORCH_CHECK(q.scalar_type() == torch::kUInt8, fn, ": ", what, " codes must be uint8");
  TORCH_CHECK(q.is_contiguous(), fn, ": ", what, " codes must be contiguous");
  TORCH_CHECK(q.numel() == rows * k, fn, ": ", what, " codes must hold rows*K values");
  TORCH_CHECK(a.device() == dev, fn, ": ", what, " absmax must be on xq's device");
  TORCH_CHECK(a.scalar_type() == torch::kFloat32, fn, ": ", what, " absmax must be fp32");
  TORCH_CHECK(a.is_contiguous(), fn, ": ", what, " absmax must be contiguous");
  TORCH_CHECK(a.numel() == rows, fn, ": ", what, " absmax must hold one value per row");
}

// xs / ws are the per-row absmax as quantize_rows_fp8 returns them; the
// kernel turns them into scales (absmax/448) itself.
// KRAG: xq is [M, Kp], Kp = K rounded up to 128, its pad columns zero codes
// (the contract of quantize_rows_fp8_padded; not checked here), wq N*K bytes.
template <bool RAGGED, bool KRAG = false>
static torch::Tensor fused_fp8_gemm_impl(const char* fn, torch::Tensor xq, torch::Tensor xs,
                                         torch::Tensor wq, torch::Tensor ws, long N, long K,
                                         torch::Tensor t, torch::Tensor bw, torch::Tensor bias,
                                         double lora_scale) {
  TORCH_CHECK(xq.is_cuda(), fn, ": xq must be a GPU tensor");
  TORCH_CHECK(xq.dim() == 2, fn, KRAG ? ": xq must be 2-D [M, Kp]" : ": xq must be 2-D [M, K]");
  const long M = xq.size(0), KA = xq.size(1);
  if (!KRAG) K = KA;
  TORCH_CHECK(M > 0 && K > 0 && N > 0, fn, ": M, N and K must be > 0");
  if (KRAG) {
    TORCH_CHECK(M % 256 == 0, fn, " requires M%256==0");
    TORCH_CHECK(K < (1L << 24) && N < (1L << 31) && (M >> 8) * ((N + 255) >> 8) < (1L << 31), fn,
                ": shape too large");
    TORCH_CHECK(KA == (K + 127) / 128 * 128, fn, ": xq must have K rounded up to 128 columns");
  } else if (RAGGED) {
    TORCH_CHECK(M % 256 == 0 && K % 128 == 0, fn, " requires M%256==0, K%128==0");
    TORCH_CHECK(N < (1L << 31) && (M >> 8) * ((N + 255) >> 8) < (1L << 31), fn,
                ": shape too large");
  } else {
    TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 128 == 0, fn,
                " requires M%256==0, N%256==0, K%128==0");
  }
  const auto dev = xq.device();
  check_fp8_operand(fn, "x", xq, xs, dev, M, KA);
  check_fp8_operand(fn, "w", wq, ws, dev, N, K);
  if (KRAG) {  // W's rows come through registers from any address
    TORCH_CHECK((uintptr_t)xq.data_ptr() % 16 == 0, fn, ": xq must be 16-byte aligned");
  } else if (RAGGED) {  // the glds staging reads 16 bytes a lane from both code tensors
    TORCH_CHECK((uintptr_t)xq.data_ptr() % 16 == 0 && (uintptr_t)wq.data_ptr() % 16 == 0, fn,
                ": code tensors must be 16-byte aligned");
  }
  const LoraArgs a = prep_lora_bias(fn, "xq", dev, t, bw, bias, M, N, 64, 256, lora_scale);
  auto y = torch::empty({M, N}, xq.options().dtype(torch::kBFloat16));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((unsigned)((M >> 8) * ((RAGGED ? N + 255 : N) >> 8))), block(512);
  const size_t smem = 4 * FP8_TILE_BYTES;  // 128 KiB
  hipLaunchKernelGGL((fused_fp8_gemm_kernel<RAGGED, KRAG>), grid, block, smem, stream,
                     xq.data_ptr<uint8_t>(), xs.data_ptr<float>(), wq.data_ptr<uint8_t>(),
                     ws.data_ptr<float>(),
                     a.t, a.bw, a.bias, (__hip_bfloat16*)y.data_ptr(), M, N, K, a.r);
  HIP_CHECK_LAST();
  return y;
}

torch::Tensor fused_fp8_gemm(torch::Tensor xq, torch::Tensor xs, torch::Tensor wq,
                             torch::Tensor ws, long N, torch::Tensor t, torch::Tensor bw,
                             torch::Tensor bias, double lora_scale) {
  return fused_fp8_gemm_impl<false>("fused_fp8_gemm", xq, xs, wq, ws, N, 0, t, bw, bias,
                                    lora_scale);
}

// fused_fp8_gemm for any N >= 1 (llama_1b's gate/up: N = 5461); y has pitch N
torch::Tensor fused_fp8_gemm_ragged(torch::Tensor xq, torch::Tensor xs, torch::Tensor wq,
                                    torch::Tensor ws, long N, torch::Tensor t,
                                    torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  return fused_fp8_gemm_impl<true>("fused_fp8_gemm_ragged", xq, xs, wq, ws, N, 0, t, bw, bias,
                                   lora_scale);
}

// ... and for any K >= 1 (llama_1b's down_proj: K = 5461) on the padded codes
// of the activations: xq / xs = quantize_rows_fp8_padded(x), wq [N,K] as stored
torch::Tensor fused_fp8_gemm_kragged(torch::Tensor xq, torch::Tensor xs, torch::Tensor wq,
                                     torch::Tensor ws, long N, long K, torch::Tensor t,
                                     torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  return fused_fp8_gemm_impl<true, true>("fused_fp8_gemm_kragged", xq, xs, wq, ws, N, K, t, bw,
                                         bias, lora_scale);
}


// ===========================================================================
// fp8 backward (`--fp8_backward`): dx = dy @ W on the e4m3 codes of W as
// stored.  dx[m,k] = sum_n dy[m,n] * code_w[n,k] * sw[n] reduces over W's
// rows, so W's row scale varies along the reduction.  It is folded into the
// gradient BEFORE that is quantised — g = dy * diag(sw) — and g gets the
// ordinary per-token-row e4m3 quantisation; the GEMM then runs on raw codes
// of both operands with one rank-1 scale (g's) in the epilogue.
//
//   quantize_rows_fp8_scaled  bf16 dy [M,N], fp32 ws [N] -> (codes, absmax)
//   fused_fp8_gemm_dx         dx = (gq · wq) · sg, bf16 out [M,K]
// ===========================================================================

struct Unit16f { float v[16]; };

// g = float(dy) * (ws/448): the quotient as fused_fp8_gemm_kernel spells sw,
// the product rounded once to fp32.  `ws16` is the unit's 64 bytes of ws.
DEV_INLINE Unit16f unit_scale(const Unit16& u, const float* __restrict__ ws16) {
  const unsigned w[8] = {u.lo.x, u.lo.y, u.lo.z, u.lo.w, u.hi.x, u.hi.y, u.hi.z, u.hi.w};
  Unit16f g;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 s = reinterpret_cast<const float4*>(ws16)[i];
    g.v[4 * i + 0] = __fmul_rn(__uint_as_float(w[2 * i] << 16), __fdiv_rn(s.x, FP8_MAX));
    g.v[4 * i + 1] = __fmul_rn(__uint_as_float(w[2 * i] & 0xffff0000u), __fdiv_rn(s.y, FP8_MAX));
    g.v[4 * i + 2] = __fmul_rn(__uint_as_float(w[2 * i + 1] << 16), __fdiv_rn(s.z, FP8_MAX));
    g.v[4 * i + 3] =
        __fmul_rn(__uint_as_float(w[2 * i + 1] & 0xffff0000u), __fdiv_rn(s.w, FP8_MAX));
  }
  return g;
}

DEV_INLINE float unitf_absmax(const Unit16f& g) {
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) am = fmaxf(am, fabsf(g.v[i]));
  return am;
}

DEV_INLINE uint4 unitf_encode(const Unit16f& g, float inv) {
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(__fmul_rn(g.v[4 * i], inv),
                                            __fmul_rn(g.v[4 * i + 1], inv), 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(__fmul_rn(g.v[4 * i + 2], inv),
                                        __fmul_rn(g.v[4 * i + 3], inv), p, true);
    o[i] = (unsigned)p;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// Geometry of quantize_rows_fp8_kernel; the scaled fp32 units (16 VGPRs each)
// stay in registers between the max reduction and the conversion.  NU == 0
// loops (N > 8192) and rebuilds g from L2 in the second pass.
// Unit c of a row of any length N, for the padded form: units wholly below N
// load like the aligned kernel's but through a 2-byte-aligned type (rows of
// odd N start anywhere), the unit that straddles N loads dy and ws element by
// element, units at or past N are zeros.
DEV_INLINE Unit16f unit_scale_ragged(const __hip_bfloat16* __restrict__ xrow,
                                     const float* __restrict__ ws, int c, int N) {
  Unit16f g;
  if (c * 16 + 16 <= N) {
    const Vec8<__hip_bfloat16> a = load8(xrow + c * 16), b = load8(xrow + c * 16 + 8);
    Unit16 u;
    __builtin_memcpy(&u.lo, &a, 16);
    __builtin_memcpy(&u.hi, &b, 16);
    g = unit_scale(u, ws + c * 16);
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = c * 16 + e;
      g.v[e] = n < N ? __fmul_rn(to_f32(xrow[n]), __fdiv_rn(ws[n], FP8_MAX)) : 0.f;
    }
  }
  return g;
}

// PAD: any N >= 1; the code rows have pitch Np = N rounded up to 128 and the
// bytes [N, Np) are zero codes, so the rows are 16-byte aligned glds sources
// and whole 128-deep reduction tiles for fused_fp8_gemm_dx_kernel<true>.
template <int G, int NU, bool PAD>
__global__ __launch_bounds__(256) void quantize_rows_fp8_scaled_kernel(
    const __hip_bfloat16* __restrict__ x, const float* __restrict__ ws,
    uint8_t* __restrict__ q, float* __restrict__ absmax, long R, int N) {
  const int gl = threadIdx.x & (G - 1);
  const long row = ((long)blockIdx.x * 256 + threadIdx.x) / G;
  const bool live = row < R;  // whole lane groups: shuffles stay inside a row
  const int Np = PAD ? (N + 127) & ~127 : N;
  const int units = Np >> 4;
  const __hip_bfloat16* xrow = x + (live ? row : 0) * N;
  const Unit16* src = reinterpret_cast<const Unit16*>(xrow);
  uint4* dst = reinterpret_cast<uint4*>(q + (live ? row : 0) * Np);
  float am = 0.f;
  if (NU > 0) {
    Unit16f g[NU > 0 ? NU : 1];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int c = gl + i * G;
      if (live && c < units) {
        g[i] = PAD ? unit_scale_ragged(xrow, ws, c, N) : unit_scale(src[c], ws + c * 16);
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) g[i].v[e] = 0.f;
      }
      am = fmaxf(am, unitf_absmax(g[i]));
    }
    am = group_max<G>(am);
    const float inv = am > 0.f ? __fdiv_rn(FP8_MAX, am) : 0.f;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int c = gl + i * G;
      if (live && c < units) dst[c] = unitf_encode(g[i], inv);
    }
  } else {
    if (live)
      for (int c = gl; c < units; c += G)
        am = fmaxf(am, unitf_absmax(PAD ? unit_scale_ragged(xrow, ws, c, N)
                                        : unit_scale(src[c], ws + c * 16)));
    am = group_max<G>(am);
    const float inv = am > 0.f ? __fdiv_rn(FP8_MAX, am) : 0.f;
    if (live)
      for (int c = gl; c < units; c += G)
        dst[c] = unitf_encode(PAD ? unit_scale_ragged(xrow, ws, c, N)
                                  : unit_scale(src[c], ws + c * 16), inv);
  }
  if (live && gl == 0) absmax[row] = am;
}

template <int G, int NU, bool PAD = false>
static void launch_quantize_scaled(const torch::Tensor& x, const torch::Tensor& ws,
                                   torch::Tensor& q, torch::Tensor& am, long R, int N,
                                   hipStream_t stream) {
  const long rows_per_block = 256 / G;
  dim3 grid((unsigned)((R + rows_per_block - 1) / rows_per_block)), block(256);
  hipLaunchKernelGGL((quantize_rows_fp8_scaled_kernel<G, NU, PAD>), grid, block, 0, stream,
                     (const __hip_bfloat16*)x.data_ptr(), ws.data_ptr<float>(),
                     q.data_ptr<uint8_t>(), am.data_ptr<float>(), R, N);
}

// dy [M,N] bf16, ws [N] = the absmax of W's rows as QuantizedWeight keeps them
template <bool PAD>
static std::vector<torch::Tensor> quantize_rows_fp8_scaled_impl(const char* fn, torch::Tensor dy,
                                                                torch::Tensor ws) {
  TORCH_CHECK(dy.is_cuda(), fn, ": dy must be a GPU tensor");
  TORCH_CHECK(dy.dim() == 2, fn, ": dy must be 2-D [M, N]");
  TORCH_CHECK(dy.is_contiguous(), fn, ": dy must be contiguous");
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16, fn, ": dy must be bf16");
  const long R = dy.size(0), N = dy.size(1);
  TORCH_CHECK(R > 0 && N > 0, fn, ": M and N must be > 0");
  if (!PAD) TORCH_CHECK(N % 16 == 0, fn, ": N must be a multiple of 16");
  TORCH_CHECK(N < (1L << 31) - (PAD ? 128 : 0) && R < (1L << 31) * 4, fn, ": shape too large");
  TORCH_CHECK(ws.device() == dy.device(), fn, ": ws must be on dy's device");
  TORCH_CHECK(ws.scalar_type() == torch::kFloat32, fn, ": ws must be fp32");
  TORCH_CHECK(ws.is_contiguous(), fn, ": ws must be contiguous");
  TORCH_CHECK(ws.numel() == N, fn, ": ws must hold one value per column of dy");
  const long Np = PAD ? (N + 127) / 128 * 128 : N;  // the form is chosen by the padded width
  auto q = torch::empty({R, Np}, dy.options().dtype(torch::kUInt8));
  auto am = torch::empty({R}, dy.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int n = (int)N;
  if (Np <= 256) {
    launch_quantize_scaled<16, 1, PAD>(dy, ws, q, am, R, n, stream);
  } else if (Np <= 1024) {
    launch_quantize_scaled<64, 1, PAD>(dy, ws, q, am, R, n, stream);
  } else if (Np <= 2048) {
    launch_quantize_scaled<64, 2, PAD>(dy, ws, q, am, R, n, stream);
  } else if (Np <= 4096) {
    launch_quantize_scaled<64, 4, PAD>(dy, ws, q, am, R, n, stream);
  } else if (Np <= 8192) {
    launch_quantize_scaled<64, 8, PAD>(dy, ws, q, am, R, n, stream);
  } else {
    launch_quantize_scaled<64, 0, PAD>(dy, ws, q, am, R, n, stream);
  }
  HIP_CHECK_LAST();
  return {q, am};
}

std::vector<torch::Tensor> quantize_rows_fp8_scaled(torch::Tensor dy, torch::Tensor ws) {
  return quantize_rows_fp8_scaled_impl<false>("quantize_rows_fp8_scaled", dy, ws);
}

// any N >= 1: codes [M, Np], Np = N rounded up to 128, the pad bytes zero codes
std::vector<torch::Tensor> quantize_rows_fp8_scaled_padded(torch::Tensor dy, torch::Tensor ws) {
  return quantize_rows_fp8_scaled_impl<true>("quantize_rows_fp8_scaled_padded", dy, ws);
}

// ---------------------------------------------------------------------------
// fused_fp8_gemm_dx.  Geometry of fused_fp8_gemm_kernel (256x256 tile over
// [M,K], 8 waves 2x4, 128-deep reduction tiles over n, double buffer, one
// vmcnt(0) + barrier per tile, XCD remap, 16x16x128 MFMA, staged b128 store).
// A = gq [M,N] is reduction-contiguous: glds staging and frag_fp8 as above.
//
// B = W [N,K] arrives transposed: a reduction tile is [128 n][256 k] bytes
// and a fragment wants 32 bytes along n.  Each thread owns one 16 n x 4 k
// patch: 16 dword loads issued one tile ahead (they fly during the MFMAs),
// a byte transposition of the four 4x4 blocks with v_perm_b32, and four
// b128 stores into a [256 k][128 n] image with the swz8 swizzle, which
// frag_fp8 then reads unchanged.
//
// Patch assignment (wave w, lane l):  k-quad q = l[1:0] | l[5:3]<<2 | w[0]<<5
// (image rows 4q..4q+3), n-chunk c = 2*w[2:1] + l[2].  An 8-lane b128 write
// group then holds 4 values of (row>>1)&7 — all of one parity — times both
// parities of c: the 8 swizzled chunks are distinct, i.e. conflict-free
// (tools/lds_bank_model.py fp8_dx_patch_writes; lane l -> rows 4l..4l+3 is
// 2-way).  A wave's dword load covers 2 rows x 128 contiguous bytes.
// ---------------------------------------------------------------------------

// bytes {S0 (4..7), S1 (0..3)} picked by the selector's four bytes
DEV_INLINE unsigned perm_b32(unsigned hi, unsigned lo, unsigned sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}

// issue the 16 dword loads of this thread's patch of one W reduction tile;
// `tile` points at W[n_tile0][k0] (uniform), `voff` is the lane's byte offset
DEV_INLINE void load_b_patch(unsigned (&st)[16], const char* tile, long K, unsigned voff) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    st[i] = *reinterpret_cast<const unsigned*>(tile + (long)i * K + voff);
}

// st[i] holds W[n = 16c + i][k = 4q .. 4q+3]; write image rows 4q..4q+3,
// 16-byte chunk c (n = 16c .. 16c+15 ascending)
DEV_INLINE void write_b_patch(char* image, const unsigned (&st)[16], int pq, int pc) {
  unsigned o[4][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const unsigned lo01 = perm_b32(st[4 * b + 1], st[4 * b + 0], 0x05010400u);
    const unsigned hi01 = perm_b32(st[4 * b + 1], st[4 * b + 0], 0x07030602u);
    const unsigned lo23 = perm_b32(st[4 * b + 3], st[4 * b + 2], 0x05010400u);
    const unsigned hi23 = perm_b32(st[4 * b + 3], st[4 * b + 2], 0x07030602u);
    o[0][b] = perm_b32(lo23, lo01, 0x05040100u);
    o[1][b] = perm_b32(lo23, lo01, 0x07060302u);
    o[2][b] = perm_b32(hi23, hi01, 0x05040100u);
    o[3][b] = perm_b32(hi23, hi01, 0x07060302u);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned p = swz8((unsigned)(4 * pq + j) * 128u + (unsigned)pc * 16u);
    *reinterpret_cast<i32x4_q*>(image + p) =
        i32x4_q{(int)o[j][0], (int)o[j][1], (int)o[j][2], (int)o[j][3]};
  }
}

// The patch of a reduction tile that holds only `nv` < 128 rows of W (the last
// tile of a ragged N).  Rows at or past nv read row nv-1 instead, so no byte
// outside W is touched; the lane offsets stay 32-bit (127*K + 252 < 2^31).
DEV_INLINE void load_b_patch_edge(unsigned (&st)[16], const char* tile, unsigned K, int pq,
                                  int pc, int nv) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int n = pc * 16 + i;
    const unsigned off = (unsigned)(n < nv ? n : nv - 1) * K + (unsigned)(pq * 4);
    st[i] = *reinterpret_cast<const unsigned*>(tile + off);
  }
}

// ... and their registers are cleared before the transposition: the clamped
// loads hold codes of a real row, and 0 x NaN-code would not be 0
DEV_INLINE void zero_b_patch_edge(unsigned (&st)[16], int pc, int nv) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (pc * 16 + i >= nv) st[i] = 0u;
}

// --- the patch for a ragged output width K (KRAG): W's rows have pitch K, so
// a patch's four k bytes at n*K + 4q are an unaligned dword ------------------

DEV_INLINE unsigned load32_any(const char* p) {
  unsigned v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

DEV_INLINE void load_b_patch_any(unsigned (&st)[16], const char* tile, long K, unsigned voff) {
#pragma unroll
  for (int i = 0; i < 16; ++i) st[i] = load32_any(tile + (long)i * K + voff);
}

// The last reduction tile: rows clamped as in load_b_patch_edge; `rows` points
// at W[n_tile0][0], `koff` is the lane's byte offset within a row and `rem`
// the bytes from `rows` to the end of wq.  The quad of W's last row that
// straddles K would end behind wq: a dword that would, is moved back to end
// with wq, and fix_b_patch_kedge shifts its bytes down by the difference (at
// most 3).  Offsets are taken from rows - 4, so that they stay unsigned when
// the tile holds fewer than 4 bytes (wq holds 4 or more).
DEV_INLINE void load_b_patch_kedge(unsigned (&st)[16], const char* rows, unsigned K,
                                   unsigned koff, int pc, int nv, unsigned rem) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int n = pc * 16 + i;
    const unsigned end = (unsigned)(n < nv ? n : nv - 1) * K + koff + 4u;
    st[i] = load32_any(rows - 4 + (end < rem ? end : rem));
  }
}

// ... and rows at or past nv are cleared, as in zero_b_patch_edge
DEV_INLINE void fix_b_patch_kedge(unsigned (&st)[16], unsigned K, unsigned koff, int pc, int nv,
                                  unsigned rem) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int n = pc * 16 + i;
    const unsigned end = (unsigned)(n < nv ? n : nv - 1) * K + koff + 4u;
    st[i] = n >= nv ? 0u : st[i] >> (end > rem ? (end - rem) * 8u : 0u);
  }
}

// RAGGED: any N >= 1.  gq has pitch Np = N rounded up to 128 with zero codes
// in [N, Np) (quantize_rows_fp8_scaled_padded), wq holds N rows.
// KRAG (with RAGGED): any K >= 1 as well; ceil(K/256) block columns.  In the
// edge column the patches with 4q at or past K are clamped to the last valid
// quad (their columns are never stored), and the bytes that the straddling
// quad picks up from the next row of W only feed columns nobody stores.
template <bool RAGGED, bool KRAG = false>
__global__ __launch_bounds__(512) void fused_fp8_gemm_dx_kernel(
    const uint8_t* __restrict__ gq,    // [M,N] e4m3 codes of dy*diag(sw)
    const float* __restrict__ ga,      // [M] absmax of its rows
    const uint8_t* __restrict__ wq,    // [N,K] e4m3 codes of W
    __hip_bfloat16* __restrict__ dx,   // [M,K]
    long M, long N, long K) {
  // one __shared__ array only (glds pipeline rule)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][A | B] = 128 KiB

  // XCD-aware blockIdx remap (bijective form), as in fused_fp8_gemm_kernel
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbk = (int)((KRAG ? K + 255 : K) >> 8);
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
  // KRAG: kw columns of this block are below K; the lane's quad clamped to the
  // last one that starts below K
  const int kw = (int)(K - k0 < 256 ? K - k0 : 256);
  const int qo = KRAG ? (pq * 4 < ((kw - 1) & ~3) ? pq * 4 : (kw - 1) & ~3) : pq * 4;
  const unsigned voff = (unsigned)(pc * 16) * (unsigned)K + (unsigned)qo;

  f32x4_q acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_q{0.f, 0.f, 0.f, 0.f};

  const char* gg = (const char*)gq;
  const char* wg = (const char*)wq + k0;
  unsigned st[16];

  const long ND = RAGGED ? (N + 127) & ~127L : N;  // pitch of gq, reduction depth
  const int NT = (int)(ND >> 7);                   // 128-n tiles
  // rows of W in the last tile; < 128 only when RAGGED
  const int nv = RAGGED ? (int)(N - ((long)(NT - 1) << 7)) : 128;
  // KRAG: the last tile takes the edge path when it is short or a quad
  // straddles K; with K < 4 every dword spans rows, so every tile takes it
  const bool kedge = KRAG && (nv < 128 || (K & 3) != 0);
  auto kedge_rem = [&](int nt_) {  // bytes from the tile's first row to the end of wq
    long l = (N - ((long)nt_ << 7)) * K;
    if (nt_ == 0 && l < 4) l = 4;  // N*K < 4: the host has padded wq to four bytes
    return (unsigned)(l < 0xffffffffL ? l : 0xffffffffL);
  };
  stage_tile_bytes(FP8_BUF_A(0), gg, m0, ND, 0, wave, lane);
  if (KRAG) {
    if ((NT == 1 && kedge) || K < 4) {
      const int nvt = NT == 1 ? nv : 128;
      load_b_patch_kedge(st, (const char*)wq, (unsigned)K, (unsigned)k0 + qo, pc, nvt, kedge_rem(0));
      fix_b_patch_kedge(st, (unsigned)K, (unsigned)k0 + qo, pc, nvt, kedge_rem(0));
    } else {
      load_b_patch_any(st, wg, K, voff);
    }
  } else if (RAGGED && NT == 1 && nv < 128) {
    load_b_patch_edge(st, wg, (unsigned)K, pq, pc, nv);
    zero_b_patch_edge(st, pc, nv);
  } else {
    load_b_patch(st, wg, K, voff);
  }
  write_b_patch(FP8_BUF_B(0), st, pq, pc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int nt = 0; nt < NT; ++nt) {
    const int cur = nt & 1;
    const bool more = nt + 1 < NT;
    // uniform: the next tile is short (KRAG: or has a quad that straddles K)
    const bool edge = RAGGED && ((nt + 2 == NT && (KRAG ? kedge : nv < 128)) || (KRAG && K < 4));
    const int nvt = nt + 2 == NT ? nv : 128;  // KRAG: rows of the next tile
    if (more) {
      stage_tile_bytes(FP8_BUF_A(cur ^ 1), gg, m0, ND, (long)(nt + 1) << 7, wave, lane);
      const char* tile = wg + ((long)(nt + 1) << 7) * K;
      if (KRAG) {
        // opaque, as below: only the quad and the chunk stay live across the
        // MFMAs, the offsets are rebuilt from them for every tile
        int qv = qo, co = pc;
        asm volatile("" : "+v"(qv), "+v"(co));
        if (edge) {
          load_b_patch_kedge(st, tile - k0, (unsigned)K, (unsigned)k0 + qv, co, nvt,
                             kedge_rem(nt + 1));
        } else {
          load_b_patch_any(st, tile, K, (unsigned)(co * 16) * (unsigned)K + (unsigned)qv);
        }
      } else if (edge) {
        int q4 = pq;  // opaque like vo below, so the 16 offsets are not hoisted
        asm volatile("" : "+v"(q4));
        load_b_patch_edge(st, tile, (unsigned)K, q4, pc, nv);
      } else {
        // keep the lane offset a 32-bit VGPR next to scalar row bases (saddr
        // form): hoisted out of the loop it becomes 16 64-bit lane addresses
        unsigned vo = voff;
        asm volatile("" : "+v"(vo));
        load_b_patch(st, tile, K, vo);
      }
    }
    const char* A = FP8_BUF_A(cur);
    const char* B = FP8_BUF_B(cur);
    __builtin_amdgcn_s_setprio(1);
    // the 4 B fragments stay resident (32 VGPRs); A fragments stream through
    i32x8_q bf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = frag_fp8(B, wc * 64 + j * 16 + fr, fq);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const i32x8_q af = frag_fp8(A, wr * 128 + i * 16 + fr, fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            af, bf[j], acc[i][j], 0 /*A e4m3*/, 0 /*B e4m3*/, 0, 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    // the other B image was last read in the previous iteration, behind its
    // barrier; the patch loads had the whole MFMA loop to land
    if (KRAG) {
      if (edge && more) {
        int qv = qo, co = pc;
        asm volatile("" : "+v"(qv), "+v"(co));
        fix_b_patch_kedge(st, (unsigned)K, (unsigned)k0 + qv, co, nvt, kedge_rem(nt + 1));
      }
    } else if (edge) {
      zero_b_patch_edge(st, pc, nv);
    }
    if (more) write_b_patch(FP8_BUF_B(cur ^ 1), st, pq, pc);
    // drain next tile's glds, then release the buffers we just read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- the one rank-1 scale, one bf16 rounding, b128 row stores through LDS
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4_q ax = *reinterpret_cast<const f32x4_q*>(ga + m0 + wr * 128 + i * 16 + fq * 4);
    const f32x4_q sg = {__fdiv_rn(ax[0], FP8_MAX), __fdiv_rn(ax[1], FP8_MAX),
                        __fdiv_rn(ax[2], FP8_MAX), __fdiv_rn(ax[3], FP8_MAX)};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] * sg;
  }
  __bf16* mine = (__bf16*)smem + wave * (128 * 64);  // 16 KiB per wave
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
    const bf16x8_q vv = *reinterpret_cast<const bf16x8_q*>(mine + row * 64 + cb);
    if (KRAG) {
      // the ragged store path of fused_fp8_gemm_kernel, pitch K
      const long col = k0 + wc * 64 + cb;
      __hip_bfloat16* dst = dx + (m0 + wr * 128 + row) * K + col;
      if (col + 8 <= K) {
        store8(dst, *reinterpret_cast<const Vec8<__hip_bfloat16>*>(&vv));
      } else {
        const __hip_bfloat16* sv = reinterpret_cast<const __hip_bfloat16*>(&vv);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < K) dst[e] = sv[e];
      }
    } else {
      *reinterpret_cast<bf16x8_q*>(dx + (m0 + wr * 128 + row) * K + k0 + wc * 64 + cb) = vv;
    }
  }
}

// N: rows of W.  Aligned: gq is [M,N].  RAGGED: gq is [M,Np], Np = N rounded up to 128.
// KRAG: any K >= 1 as well, wq from any address.
template <bool RAGGED, bool KRAG = false>
static torch::Tensor fused_fp8_gemm_dx_impl(const char* fn, torch::Tensor gq, torch::Tensor gs,
                                            torch::Tensor wq, long N, long K) {
  TORCH_CHECK(gq.is_cuda(), fn, ": gq must be a GPU tensor");
  TORCH_CHECK(gq.dim() == 2, fn, RAGGED ? ": gq must be 2-D [M, Np]" : ": gq must be 2-D [M, N]");
  const long M = gq.size(0), ND = gq.size(1);
  if (!RAGGED) N = ND;
  TORCH_CHECK(M > 0 && N > 0 && K > 0, fn, ": M, N and K must be > 0");
  if (RAGGED) {
    TORCH_CHECK(M % 256 == 0 && (KRAG || K % 256 == 0), fn,
                KRAG ? " requires M%256==0" : " requires M%256==0, K%256==0");
    TORCH_CHECK(N < (1L << 31) - 128, fn, ": shape too large");
    TORCH_CHECK(ND == (N + 127) / 128 * 128, fn, ": gq must have N rounded up to 128 columns");
  } else {
    TORCH_CHECK(M % 256 == 0 && K % 256 == 0 && N % 128 == 0, fn,
                " requires M%256==0, K%256==0, N%128==0");
  }
  const long nbk = (KRAG ? K + 255 : K) >> 8;
  TORCH_CHECK(K < (1L << 24) && N < (1L << 31) && (M >> 8) * nbk < (1L << 31), fn,
              ": shape too large");
  const auto dev = gq.device();
  check_fp8_operand(fn, "g", gq, gs, dev, M, ND);
  TORCH_CHECK(wq.is_cuda() && wq.device() == dev, fn, ": w codes must be on gq's GPU");
  TORCH_CHECK(wq.scalar_type() == torch::kUInt8, fn, ": w codes must be uint8");
  TORCH_CHECK(wq.is_contiguous(), fn, ": w codes must be contiguous");
  TORCH_CHECK(wq.numel() == N * K, fn, ": w codes must hold N*K values");
  if (KRAG && N * K < 4)  // the patches are dword loads: give the kernel four bytes to read
    wq = torch::cat({wq.flatten(), torch::zeros({4 - N * K}, wq.options())});
  // KRAG: W's patches are unaligned dwords whatever wq's address
  TORCH_CHECK((uintptr_t)gq.data_ptr() % 16 == 0 && (KRAG || (uintptr_t)wq.data_ptr() % 16 == 0),
              fn, KRAG ? ": gq must be 16-byte aligned" : ": code tensors must be 16-byte aligned");
  auto dx = torch::empty({M, K}, gq.options().dtype(torch::kBFloat16));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((unsigned)((M >> 8) * nbk)), block(512);
  const size_t smem = 4 * FP8_TILE_BYTES;  // 128 KiB
  hipLaunchKernelGGL((fused_fp8_gemm_dx_kernel<RAGGED, KRAG>), grid, block, smem, stream,
                     gq.data_ptr<uint8_t>(), gs.data_ptr<float>(), wq.data_ptr<uint8_t>(),
                     (__hip_bfloat16*)dx.data_ptr(), M, N, K);
  HIP_CHECK_LAST();
  return dx;
}

// gq / gs: quantize_rows_fp8_scaled(dy, W's absmax); wq: W's codes [N,K]
torch::Tensor fused_fp8_gemm_dx(torch::Tensor gq, torch::Tensor gs, torch::Tensor wq, long K) {
  return fused_fp8_gemm_dx_impl<false>("fused_fp8_gemm_dx", gq, gs, wq, 0, K);
}

// gq / gs: quantize_rows_fp8_scaled_padded(dy, W's absmax), [M, ceil128(N)]; wq: [N,K]
torch::Tensor fused_fp8_gemm_dx_ragged(torch::Tensor gq, torch::Tensor gs, torch::Tensor wq,
                                       long N, long K) {
  return fused_fp8_gemm_dx_impl<true>("fused_fp8_gemm_dx_ragged", gq, gs, wq, N, K);
}

// ... and for any K >= 1 (llama_1b's down_proj: dx is [M, 5461]); dx has pitch K
torch::Tensor fused_fp8_gemm_dx_kragged(torch::Tensor gq, torch::Tensor gs, torch::Tensor wq,
                                        long N, long K) {
  return fused_fp8_gemm_dx_impl<true, true>("fused_fp8_gemm_dx_kragged", gq, gs, wq, N, K);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
