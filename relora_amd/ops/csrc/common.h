// Common helpers for relora_amd gfx950 (CDNA4/MI355X) kernels.
// Wave size is 64 on CDNA4; block sizes are multiples of 64.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
#define DEV_INLINE __device__ __forceinline__

// ---- scalar conversions ---------------------------------------------------

DEV_INLINE float to_f32(float x) { return x; }
DEV_INLINE float to_f32(__hip_bfloat16 x) { return __bfloat162float(x); }

template <typename T> DEV_INLINE T from_f32(float x);
template <> DEV_INLINE float from_f32<float>(float x) { return x; }
template <> DEV_INLINE __hip_bfloat16 from_f32<__hip_bfloat16>(float x) {
  return __float2bfloat16(x);
}

// ---- vector types: 8 consecutive elements (16B for bf16, 32B for f32) -----
// bf16 loads MUST be vectorized on CDNA4 (guide G13): scalar bf16 ~2-2.5x slower.

template <typename T> struct Vec8 { T v[8]; };

template <typename T>
DEV_INLINE Vec8<T> load8(const T* p) {
  return *reinterpret_cast<const Vec8<T>*>(p);
}
template <typename T>
DEV_INLINE void store8(T* p, const Vec8<T>& x) {
  *reinterpret_cast<Vec8<T>*>(p) = x;
}

// ---- RoPE rotation of one (x1, x2) = (x[i], x[i + R/2]) pair -----------------
// forward:  y1 = x1*c - x2*s,  y2 = x2*c + x1*s
// inverse:  y1 = x1*c + x2*s,  y2 = x2*c - x1*s   (the backward rotation)
// Shared by rope_kernel, rope_vec_kernel (rope.hip) and the fused LoRA + RoPE
// epilogue (lora_gemm.hip).  Of the two products of each line one is rounded
// to fp32 and the other fused into the add.  Which one is spelled out, so that
// every caller rounds alike whatever the compiler would contract on its own;
// the choice is the one the compiler made for rope_kernel while these lines
// were written `x1 * c - x2 * s` etc. (read off its ISA), so results did not
// move when the helper came in.

template <bool INVERSE>
DEV_INLINE void rope_rotate(float x1, float x2, float c, float s, float& y1, float& y2) {
  if (INVERSE) {
    y1 = fmaf(x1, c, __fmul_rn(x2, s));
    y2 = fmaf(x2, c, -__fmul_rn(x1, s));
  } else {
    y1 = fmaf(x1, c, -__fmul_rn(x2, s));
    y2 = fmaf(x1, s, __fmul_rn(x2, c));
  }
}

// ---- block-level reduction (sum) over fp32 --------------------------------
// One value per thread -> one value broadcast to all threads.
// Requires blockDim.x <= 1024, caller provides __shared__ float scratch[16].

DEV_INLINE float wave_reduce_sum(float x) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_down(x, off);
  return x;  // valid in lane 0
}

DEV_INLINE float block_reduce_sum(float x, float* scratch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int nwaves = (blockDim.x + WAVE - 1) / WAVE;
  x = wave_reduce_sum(x);
  if (lane == 0) scratch[wid] = x;
  __syncthreads();
  float total = 0.f;
  if (wid == 0) {
    float v = (lane < nwaves) ? scratch[lane] : 0.f;
    v = wave_reduce_sum(v);
    if (lane == 0) scratch[0] = v;
  }
  __syncthreads();
  total = scratch[0];
  __syncthreads();
  return total;
}

DEV_INLINE float wave_reduce_max(float x) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x = fmaxf(x, __shfl_down(x, off));
  return x;
}

DEV_INLINE float block_reduce_max(float x, float* scratch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int nwaves = (blockDim.x + WAVE - 1) / WAVE;
  x = wave_reduce_max(x);
  if (lane == 0) scratch[wid] = x;
  __syncthreads();
  if (wid == 0) {
    float v = (lane < nwaves) ? scratch[lane] : -INFINITY;
    v = wave_reduce_max(v);
    if (lane == 0) scratch[0] = v;
  }
  __syncthreads();
  float total = scratch[0];
  __syncthreads();
  return total;
}

#define HIP_CHECK_LAST()                                                     \
  do {                                                                       \
    hipError_t e = hipGetLastError();                                        \
    TORCH_CHECK(e == hipSuccess, "HIP kernel launch failed: ",               \
                hipGetErrorString(e));                                       \
  } while (0)
