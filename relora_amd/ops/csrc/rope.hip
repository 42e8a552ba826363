#include "hip/hip_runtime.h"
// RoPE apply (K4), rotate-half convention with fp32 cos/sin tables
// (reference modeling_llama.py:126-141; partial rotary for pythia
// modeling_pythia.py:184-197). One kernel handles q and k; INVERSE=true
// computes the backward rotation (dq = dy*cos + rot_inv(dy*sin)).
//
// Layout: x [B, nh, S, hd] — BHSD-contiguous or a transposed view of a
// BSHD buffer (`x.view(B,S,nh,hd).transpose(1,2)`); the strided form lets
// the whole q/k path from the QKV projection through attention run with
// ZERO permute/contiguous copies.  cos/sin [S_cache, R] fp32 with
// duplicated halves (cos[i] == cos[i + R/2]); R <= hd, pass-through tail.
//
// Two kernels, one arithmetic (rope_rotate in common.h, identical bits):
//   rope_vec_kernel  bf16, (R/2) % 8 == 0, hd % 8 == 0, 16-byte aligned
//                    strides and pointers: q AND k in one launch, 16 bytes per
//                    access, the tail copied by the same launch
//   rope_kernel      everything else (fp32, R/2 not a multiple of 8, odd
//                    strides): one thread per pair, one launch per tensor

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"

template <typename T, bool INVERSE>
__global__ void rope_kernel(const T* __restrict__ x, T* __restrict__ y,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t,
                            int S, int hd, int R, long total_rows,
                            int nh, long bst, long hst, long ld) {
  // one thread per (row, i) pair with i < R/2; rows = B*nh*S
  const int half = R / 2;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long npairs = total_rows * half;
  if (idx >= npairs) return;
  const long row = idx / half;
  const int i = idx % half;
  const long s = row % S;  // position within sequence
  const long h = (row / S) % nh;
  const long b = row / ((long)S * nh);
  const long off = b * bst + h * hst + s * ld;

  const float c = cos_t[s * R + i];
  const float sn = sin_t[s * R + i];
  const T* xr = x + off;
  T* yr = y + off;
  const float x1 = to_f32(xr[i]);
  const float x2 = to_f32(xr[i + half]);
  float y1, y2;
  rope_rotate<INVERSE>(x1, x2, c, sn, y1, y2);
  yr[i] = from_f32<T>(y1);
  yr[i + half] = from_f32<T>(y2);
}

template <typename T>
__global__ void copy_tail_kernel(const T* __restrict__ x, T* __restrict__ y,
                                 int hd, int R, long total_rows,
                                 int S, int nh, long bst, long hst, long ld) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int tail = hd - R;
  const long n = total_rows * tail;
  if (idx >= n) return;
  const long row = idx / tail;
  const int i = R + idx % tail;
  const long s = row % S;
  const long h = (row / S) % nh;
  const long b = row / ((long)S * nh);
  const long off = b * bst + h * hst + s * ld;
  y[off + i] = x[off + i];
}

// ---------------------------------------------------------------------------
// Vectorised form.  A row of hd elements is cut into units of 8: the R/16
// units of the first rotary half, each handled together with its partner R/2
// further on (two bf16x8 loads, 32 bytes each of cos and sin, two bf16x8
// stores), then the (hd - R)/8 units of the pass-through tail (a 16-byte
// copy).  One thread per unit; the units of q come first, then those of k, so
// the two tensors (different head counts and strides: grouped-query attention)
// share one launch.  Rows are numbered in memory order — (b, s, h) for the
// transposed-BSHD view, (b, h, s) for BHSD — so a wave touches one contiguous
// stretch of memory.
// ---------------------------------------------------------------------------

struct RopeVecTensor {
  const __hip_bfloat16* x;
  __hip_bfloat16* y;
  long bst, hst, ld;  // element strides of batch, head and position
  int nh;
  int s_major;        // rows run (b, s, h): the transposed-BSHD view
};

struct RopeVecArgs {
  RopeVecTensor q, k;
  long q_units;  // units of q; k's follow
  long units;    // q's and k's together
};

template <bool INVERSE>
__global__ __launch_bounds__(256) void rope_vec_kernel(
    RopeVecArgs a, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int S, int hd, int R) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.units) return;
  const bool is_k = idx >= a.q_units;
  if (is_k) idx -= a.q_units;
  const __hip_bfloat16* x = is_k ? a.k.x : a.q.x;
  __hip_bfloat16* y = is_k ? a.k.y : a.q.y;
  const long bst = is_k ? a.k.bst : a.q.bst;
  const long hst = is_k ? a.k.hst : a.q.hst;
  const long ld = is_k ? a.k.ld : a.q.ld;
  const int nh = is_k ? a.k.nh : a.q.nh;
  const bool s_major = is_k ? a.k.s_major : a.q.s_major;

  const int half = R / 2;
  const int rot_units = half / 8;
  const int row_units = rot_units + (hd - R) / 8;
  const long row = idx / row_units;
  const int u = (int)(idx % row_units);
  long b, h, s;
  if (s_major) {
    h = row % nh;
    s = (row / nh) % S;
    b = row / ((long)nh * S);
  } else {
    s = row % S;
    h = (row / S) % nh;
    b = row / ((long)S * nh);
  }
  const long off = b * bst + h * hst + s * ld;

  if (u >= rot_units) {  // pass-through tail
    const int c = R + (u - rot_units) * 8;
    store8(y + off + c, load8(x + off + c));
    return;
  }
  const int i = u * 8;
  const Vec8<__hip_bfloat16> x1 = load8(x + off + i);
  const Vec8<__hip_bfloat16> x2 = load8(x + off + i + half);
  const Vec8<float> c = load8(cos_t + s * R + i);
  const Vec8<float> sn = load8(sin_t + s * R + i);
  Vec8<__hip_bfloat16> y1, y2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float r1, r2;
    rope_rotate<INVERSE>(to_f32(x1.v[j]), to_f32(x2.v[j]), c.v[j], sn.v[j], r1, r2);
    y1.v[j] = from_f32<__hip_bfloat16>(r1);
    y2.v[j] = from_f32<__hip_bfloat16>(r2);
  }
  store8(y + off + i, y1);
  store8(y + off + i + half, y2);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what rope_vec_kernel needs of one tensor besides bf16: 16-byte accesses
static bool rope_vec_tensor_ok(const torch::Tensor& x) {
  return x.stride(0) % 8 == 0 && x.stride(1) % 8 == 0 && x.stride(2) % 8 == 0 &&
         aligned16(x.data_ptr());
}

static RopeVecTensor rope_vec_tensor(const torch::Tensor& x, torch::Tensor& y) {
  RopeVecTensor t;
  t.x = (const __hip_bfloat16*)x.data_ptr();
  t.y = (__hip_bfloat16*)y.data_ptr();
  t.bst = x.stride(0);
  t.hst = x.stride(1);
  t.ld = x.stride(2);
  t.nh = (int)x.size(1);
  t.s_major = x.stride(1) < x.stride(2);
  return t;
}

static void rope_vec_launch(const torch::Tensor& q, torch::Tensor& qo,
                            const torch::Tensor& k, torch::Tensor& ko,
                            const torch::Tensor& cos_t, const torch::Tensor& sin_t,
                            bool inverse, hipStream_t stream) {
  const int S = q.size(2);
  const int hd = q.size(3);
  const int R = cos_t.size(1);
  const long row_units = R / 16 + (hd - R) / 8;
  RopeVecArgs a;
  a.q = rope_vec_tensor(q, qo);
  a.k = rope_vec_tensor(k, ko);
  a.q_units = (long)q.size(0) * q.size(1) * S * row_units;
  a.units = a.q_units + (long)k.size(0) * k.size(1) * S * row_units;
  if (a.units == 0) return;
  dim3 block(256), grid((a.units + 255) / 256);
  if (inverse)
    hipLaunchKernelGGL(rope_vec_kernel<true>, grid, block, 0, stream, a,
                       cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), S, hd, R);
  else
    hipLaunchKernelGGL(rope_vec_kernel<false>, grid, block, 0, stream, a,
                       cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), S, hd, R);
}

template <typename T>
static void rope_launch(const torch::Tensor& x, torch::Tensor& y,
                        const torch::Tensor& cos_t, const torch::Tensor& sin_t,
                        bool inverse, hipStream_t stream) {
  const int nh = x.size(1);
  const int S = x.size(2);
  const int hd = x.size(3);
  const int R = cos_t.size(1);
  const long bst = x.stride(0), hst = x.stride(1), ld = x.stride(2);
  const long rows = (long)x.size(0) * nh * S;
  const long npairs = rows * (R / 2);
  if (npairs == 0) return;
  dim3 block(256);
  dim3 grid((npairs + 255) / 256);
  if (inverse)
    hipLaunchKernelGGL((rope_kernel<T, true>), grid, block, 0, stream,
                       (const T*)x.data_ptr(), (T*)y.data_ptr(),
                       cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), S, hd, R,
                       rows, nh, bst, hst, ld);
  else
    hipLaunchKernelGGL((rope_kernel<T, false>), grid, block, 0, stream,
                       (const T*)x.data_ptr(), (T*)y.data_ptr(),
                       cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), S, hd, R,
                       rows, nh, bst, hst, ld);
  if (R < hd) {
    const long n = rows * (hd - R);
    hipLaunchKernelGGL(copy_tail_kernel<T>, dim3((n + 255) / 256), block, 0, stream,
                       (const T*)x.data_ptr(), (T*)y.data_ptr(), hd, R, rows,
                       S, nh, bst, hst, ld);
  }
}

static bool rope_layout_ok(const torch::Tensor& q) {
  if (q.stride(3) != 1) return false;
  const long nh = q.size(1), S = q.size(2), hd = q.size(3);
  return q.is_contiguous() ||
         (q.stride(1) == hd && q.stride(2) == nh * hd && q.stride(0) == S * nh * hd);
}

std::vector<torch::Tensor> rope_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor cos_t, torch::Tensor sin_t,
                                    bool inverse, bool force_scalar) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4);
  TORCH_CHECK(rope_layout_ok(q), "rope: unsupported q layout");
  // k may carry fewer heads than q (grouped-query attention): same B, S and
  // hd, a valid layout of its own — the kernels take head count and strides
  // per tensor.  A k without heads ([B, 0, S, hd]) rotates q alone
  TORCH_CHECK(k.is_cuda() && k.dim() == 4 && k.scalar_type() == q.scalar_type(),
              "rope: k must be a 4-d tensor of q's dtype and device");
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(2) == q.size(2) && k.size(3) == q.size(3),
              "rope: q and k must agree on batch, sequence and head_dim");
  TORCH_CHECK(rope_layout_ok(k), "rope: unsupported k layout");
  TORCH_CHECK(cos_t.is_cuda() && cos_t.dim() == 2 &&
              cos_t.scalar_type() == torch::kFloat32 && cos_t.is_contiguous());
  TORCH_CHECK(sin_t.is_cuda() && sin_t.scalar_type() == torch::kFloat32 &&
              sin_t.is_contiguous() && sin_t.sizes() == cos_t.sizes(),
              "rope: sin must match cos (fp32, contiguous, same shape)");
  TORCH_CHECK(cos_t.size(0) >= q.size(2), "rope cache shorter than sequence");
  TORCH_CHECK(cos_t.size(1) % 2 == 0 && cos_t.size(1) <= q.size(3),
              "rope: rotary width must be even and at most head_dim");
  auto qo = torch::empty_strided(q.sizes(), q.strides(), q.options());
  auto ko = torch::empty_strided(k.sizes(), k.strides(), k.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const long hd = q.size(3), R = cos_t.size(1);
  // force_scalar: the tests compare the two kernels on the same data
  const bool vec = !force_scalar && q.scalar_type() == torch::kBFloat16 &&
                   (R / 2) % 8 == 0 && hd % 8 == 0 &&
                   rope_vec_tensor_ok(q) && rope_vec_tensor_ok(k) &&
                   aligned16(cos_t.data_ptr()) && aligned16(sin_t.data_ptr());
  if (vec) {
    rope_vec_launch(q, qo, k, ko, cos_t, sin_t, inverse, stream);
  } else if (q.scalar_type() == torch::kBFloat16) {
    rope_launch<__hip_bfloat16>(q, qo, cos_t, sin_t, inverse, stream);
    rope_launch<__hip_bfloat16>(k, ko, cos_t, sin_t, inverse, stream);
  } else {
    rope_launch<float>(q, qo, cos_t, sin_t, inverse, stream);
    rope_launch<float>(k, ko, cos_t, sin_t, inverse, stream);
  }
  HIP_CHECK_LAST();
  return {qo, ko};
}
