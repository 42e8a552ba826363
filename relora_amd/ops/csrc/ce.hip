#include "hip/hip_runtime.h"
// Fused cross-entropy row kernels (K10): one-pass online max+sumexp row
// stats and the in-place softmax-minus-onehot gradient. The LM-head GEMMs
// run in hipBLASLt (library GEMMs); these kernels remove the 3 extra fp32
// passes over the [chunk, V] logits that torch's logsumexp/softmax would
// cost, and the full [M, V] logits are never materialized (the memory hot
// spot the reference flags at modeling_llama.py:696-697).

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"

// per-row online max/sumexp + target-logit gather.
template <typename T>
__global__ void ce_row_stats_kernel(const T* __restrict__ logits,
                                    const long* __restrict__ labels,
                                    float* __restrict__ lse_out,
                                    float* __restrict__ tgt_out,
                                    int V, long ignore_index) {
  __shared__ float scratch[16];
  const long row = blockIdx.x;
  const T* lr = logits + row * (long)V;

  float m = -INFINITY, s = 0.f;
  const int vec_end = (V / 8) * 8;
  for (int i = threadIdx.x * 8; i < vec_end; i += blockDim.x * 8) {
    Vec8<T> v = load8(lr + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = to_f32(v.v[j]);
      if (f > m) {
        s *= __expf(m - f);
        m = f;
      }
      s += __expf(f - m);
    }
  }
  for (int i = vec_end + threadIdx.x; i < V; i += blockDim.x) {
    float f = to_f32(lr[i]);
    if (f > m) {
      s *= __expf(m - f);
      m = f;
    }
    s += __expf(f - m);
  }
  // combine (m, s) across the block: global max then rescaled sums
  float gm = block_reduce_max(m, scratch);
  float gs = block_reduce_sum(s * __expf(m - gm), scratch);

  if (threadIdx.x == 0) {
    lse_out[row] = gm + __logf(gs);
    long lab = labels[row];
    tgt_out[row] = (lab == ignore_index) ? 0.f : to_f32(lr[lab]);
  }
}

// in place: logits[row] <- (softmax(logits[row]) - onehot(label)) * gscale
template <typename T>
__global__ void ce_grad_kernel(T* __restrict__ logits, const long* __restrict__ labels,
                               const float* __restrict__ lse, float gscale,
                               long M, int V, long ignore_index) {
  const long row = blockIdx.x;
  T* lr = logits + row * (long)V;
  const long lab = labels[row];
  const bool valid = lab != ignore_index;
  const float l = lse[row];

  const int vec_end = (V / 8) * 8;
  for (int i = threadIdx.x * 8; i < vec_end; i += blockDim.x * 8) {
    Vec8<T> v = load8(lr + i);
    Vec8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float p = valid ? __expf(to_f32(v.v[j]) - l) : 0.f;
      if (valid && (long)(i + j) == lab) p -= 1.f;
      o.v[j] = from_f32<T>(p * gscale);
    }
    store8(lr + i, o);
  }
  for (int i = vec_end + threadIdx.x; i < V; i += blockDim.x) {
    float p = valid ? __expf(to_f32(lr[i]) - l) : 0.f;
    if (valid && (long)i == lab) p -= 1.f;
    lr[i] = from_f32<T>(p * gscale);
  }
}

// ---- loss options: z-loss and label smoothing --------------------------------
// Per valid row, with smoothing eps and z coefficient z:
//   loss_row   = lse - (1-eps)*x_t - (eps/V)*sum_j x_j + z*lse^2
//   dloss/dx_j = (1 + 2*z*lse)*p_j - (1-eps)*[j == t] - eps/V
// The two kernels below are the option-carrying siblings of the plain ones
// above (same geometry: one 512-thread block per row, Vec8 body + scalar
// tail); the plain kernels stay as they are and serve the default path.

// row stats + fp32 row sum (the label-smoothing term) in the same pass.
template <typename T>
__global__ void ce_row_stats_ex_kernel(const T* __restrict__ logits,
                                       const long* __restrict__ labels,
                                       float* __restrict__ lse_out,
                                       float* __restrict__ tgt_out,
                                       float* __restrict__ sum_out,
                                       int V, long ignore_index) {
  __shared__ float scratch[16];
  const long row = blockIdx.x;
  const T* lr = logits + row * (long)V;

  float m = -INFINITY, s = 0.f, sx = 0.f;
  const int vec_end = (V / 8) * 8;
  for (int i = threadIdx.x * 8; i < vec_end; i += blockDim.x * 8) {
    Vec8<T> v = load8(lr + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = to_f32(v.v[j]);
      sx += f;
      if (f > m) {
        s *= __expf(m - f);
        m = f;
      }
      s += __expf(f - m);
    }
  }
  for (int i = vec_end + threadIdx.x; i < V; i += blockDim.x) {
    float f = to_f32(lr[i]);
    sx += f;
    if (f > m) {
      s *= __expf(m - f);
      m = f;
    }
    s += __expf(f - m);
  }
  float gm = block_reduce_max(m, scratch);
  float gs = block_reduce_sum(s * __expf(m - gm), scratch);
  float gx = block_reduce_sum(sx, scratch);

  if (threadIdx.x == 0) {
    lse_out[row] = gm + __logf(gs);
    long lab = labels[row];
    // an out-of-range label reads nothing (torch's CE would raise on it)
    tgt_out[row] = (lab == ignore_index || lab < 0 || lab >= V) ? 0.f : to_f32(lr[lab]);
    sum_out[row] = gx;
  }
}

// in place: logits[row] <- ((1 + 2*z*lse)*softmax - (1-eps)*onehot - eps/V) * gscale
template <typename T>
__global__ void ce_grad_ex_kernel(T* __restrict__ logits, const long* __restrict__ labels,
                                  const float* __restrict__ lse, float gscale,
                                  float z, float eps, long M, int V, long ignore_index) {
  const long row = blockIdx.x;
  T* lr = logits + row * (long)V;
  const long lab = labels[row];
  const bool valid = lab != ignore_index;
  const float l = lse[row];
  const float coef = 1.f + 2.f * z * l;
  const float hot = 1.f - eps;
  const float uni = eps / (float)V;

  const int vec_end = (V / 8) * 8;
  for (int i = threadIdx.x * 8; i < vec_end; i += blockDim.x * 8) {
    Vec8<T> v = load8(lr + i);
    Vec8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = 0.f;
      if (valid) {
        g = coef * __expf(to_f32(v.v[j]) - l) - uni;
        if ((long)(i + j) == lab) g -= hot;
      }
      o.v[j] = from_f32<T>(g * gscale);
    }
    store8(lr + i, o);
  }
  for (int i = vec_end + threadIdx.x; i < V; i += blockDim.x) {
    float g = 0.f;
    if (valid) {
      g = coef * __expf(to_f32(lr[i]) - l) - uni;
      if ((long)i == lab) g -= hot;
    }
    lr[i] = from_f32<T>(g * gscale);
  }
}

std::vector<torch::Tensor> ce_row_stats(torch::Tensor logits, torch::Tensor labels,
                                        long ignore_index) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(labels.scalar_type() == torch::kInt64);
  const long M = logits.size(0);
  const int V = logits.size(1);
  auto lse = torch::empty({M}, logits.options().dtype(torch::kFloat32));
  auto tgt = torch::empty({M}, logits.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(M), block(512);
  if (logits.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(ce_row_stats_kernel<__hip_bfloat16>, grid, block, 0, stream,
                       (const __hip_bfloat16*)logits.data_ptr(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), tgt.data_ptr<float>(), V, ignore_index);
  else
    hipLaunchKernelGGL(ce_row_stats_kernel<float>, grid, block, 0, stream,
                       logits.data_ptr<float>(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), tgt.data_ptr<float>(), V, ignore_index);
  HIP_CHECK_LAST();
  return {lse, tgt};
}

void ce_grad_(torch::Tensor logits, torch::Tensor labels, torch::Tensor lse,
              double gscale, long ignore_index) {
  const long M = logits.size(0);
  const int V = logits.size(1);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(M), block(512);
  if (logits.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(ce_grad_kernel<__hip_bfloat16>, grid, block, 0, stream,
                       (__hip_bfloat16*)logits.data_ptr(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), (float)gscale, M, V, ignore_index);
  else
    hipLaunchKernelGGL(ce_grad_kernel<float>, grid, block, 0, stream,
                       logits.data_ptr<float>(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), (float)gscale, M, V, ignore_index);
  HIP_CHECK_LAST();
}

static void check_ce_logits(const torch::Tensor& logits, const torch::Tensor& labels) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16 ||
              logits.scalar_type() == torch::kFloat32, "ce: logits must be bf16 or fp32");
  TORCH_CHECK(labels.scalar_type() == torch::kInt64);
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() && labels.dim() == 1 &&
              labels.size(0) == logits.size(0), "ce: labels must be a contiguous [M] tensor");
}

std::vector<torch::Tensor> ce_row_stats_ex(torch::Tensor logits, torch::Tensor labels,
                                           long ignore_index) {
  check_ce_logits(logits, labels);
  const long M = logits.size(0);
  const int V = logits.size(1);
  auto lse = torch::empty({M}, logits.options().dtype(torch::kFloat32));
  auto tgt = torch::empty({M}, logits.options().dtype(torch::kFloat32));
  auto rsum = torch::empty({M}, logits.options().dtype(torch::kFloat32));
  if (M == 0) return {lse, tgt, rsum};
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(M), block(512);
  if (logits.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(ce_row_stats_ex_kernel<__hip_bfloat16>, grid, block, 0, stream,
                       (const __hip_bfloat16*)logits.data_ptr(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), tgt.data_ptr<float>(), rsum.data_ptr<float>(),
                       V, ignore_index);
  else
    hipLaunchKernelGGL(ce_row_stats_ex_kernel<float>, grid, block, 0, stream,
                       logits.data_ptr<float>(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), tgt.data_ptr<float>(), rsum.data_ptr<float>(),
                       V, ignore_index);
  HIP_CHECK_LAST();
  return {lse, tgt, rsum};
}

void ce_grad_ex_(torch::Tensor logits, torch::Tensor labels, torch::Tensor lse,
                 double gscale, double z_loss, double label_smoothing, long ignore_index) {
  check_ce_logits(logits, labels);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat32 && lse.is_contiguous() &&
              lse.dim() == 1 && lse.size(0) == logits.size(0),
              "ce: lse must be a contiguous fp32 [M] tensor");
  TORCH_CHECK(z_loss >= 0.0, "ce: z_loss must be >= 0");
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing < 1.0,
              "ce: label_smoothing must be in [0, 1)");
  const long M = logits.size(0);
  const int V = logits.size(1);
  if (M == 0) return;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(M), block(512);
  if (logits.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(ce_grad_ex_kernel<__hip_bfloat16>, grid, block, 0, stream,
                       (__hip_bfloat16*)logits.data_ptr(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), (float)gscale, (float)z_loss,
                       (float)label_smoothing, M, V, ignore_index);
  else
    hipLaunchKernelGGL(ce_grad_ex_kernel<float>, grid, block, 0, stream,
                       logits.data_ptr<float>(), labels.data_ptr<long>(),
                       lse.data_ptr<float>(), (float)gscale, (float)z_loss,
                       (float)label_smoothing, M, V, ignore_index);
  HIP_CHECK_LAST();
}
