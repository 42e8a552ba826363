#include "hip/hip_runtime.h"
// AdamW for bf16 parameters with fp32 moments and/or stochastic rounding
// (the `_ex` companion of adamw.hip; the plain kernels there are untouched
// and remain the default path). Same chunk-table / grid-stride geometry and
// the same fp32 math as the plain pair. S is the moment dtype; SR selects
// stochastic rounding for every bf16 destination. fp32 moments are stored
// unrounded. The random bits come from Philox4x32-10 keyed by the seed with
// counter (element index, step, tensor ordinal): one call per element, and
// nothing depends on which kernel or grid processed the element.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"
#include "philox4x32.h"

#define MT_MAX 48
#define MT_CHUNK 65536
#define MT_BLOCKS 320

struct AdamWExArgs {
  void* p[MT_MAX];
  void* g[MT_MAX];
  void* m[MT_MAX];
  void* v[MT_MAX];
  long numel[MT_MAX];
  uint32_t ordinal[MT_MAX];                  // Philox counter word 3
  unsigned char tensor_of_block[MT_BLOCKS];  // which tensor a block belongs to
  int chunk_of_block[MT_BLOCKS];             // chunk INDEX within that tensor
};
static_assert(sizeof(AdamWExArgs) + 64 <= 4096, "kernel argument block must stay under 4 KB");

struct AdamWExScalars {
  float lr, beta1, beta2, eps, wd, bc1, bc2;
  uint32_t seed_lo, seed_hi, step;
};

template <typename S, bool SR>
DEV_INLINE S round_dest(float x, uint32_t r16) {
  if constexpr (std::is_same<S, float>::value) {
    return x;
  } else if constexpr (SR) {
    return stochastic_round_bf16(x, r16);
  } else {
    return from_f32<S>(x);
  }
}

// One element; `index` is the element's index within its tensor.
template <typename S, bool SR>
DEV_INLINE void adamw_ex_element(__hip_bfloat16* p, const __hip_bfloat16* g, S* m, S* v,
                                 long i, long index, uint32_t ordinal, float decay,
                                 float step_size, float inv_bc2, const AdamWExScalars& s) {
  float pf = to_f32(p[i]) * decay;
  float gf = to_f32(g[i]);
  float mf = s.beta1 * to_f32(m[i]) + (1.f - s.beta1) * gf;
  float vf = s.beta2 * to_f32(v[i]) + (1.f - s.beta2) * gf * gf;
  Philox4 r = {};
  if constexpr (SR) r = philox_for_element(s.seed_lo, s.seed_hi, index, s.step, ordinal);
  m[i] = round_dest<S, SR>(mf, philox_lane16(r, 1));
  v[i] = round_dest<S, SR>(vf, philox_lane16(r, 2));
  const float denom = sqrtf(vf * inv_bc2) + s.eps;
  p[i] = round_dest<__hip_bfloat16, SR>(pf - step_size * mf / denom, philox_lane16(r, 0));
}

template <typename S, bool SR>
__global__ void fused_adamw_ex_kernel(AdamWExArgs args, AdamWExScalars s) {
  const int t = args.tensor_of_block[blockIdx.x];
  const long start = (long)args.chunk_of_block[blockIdx.x] * MT_CHUNK;
  const long n = args.numel[t];
  __hip_bfloat16* p = (__hip_bfloat16*)args.p[t] + start;
  const __hip_bfloat16* g = (const __hip_bfloat16*)args.g[t] + start;
  S* m = (S*)args.m[t] + start;
  S* v = (S*)args.v[t] + start;
  const uint32_t ordinal = args.ordinal[t];
  const long n_rem = n - start;
  const long len = n_rem < MT_CHUNK ? n_rem : MT_CHUNK;

  const float decay = 1.f - s.lr * s.wd;
  const float step_size = s.lr / s.bc1;
  const float inv_bc2 = 1.f / s.bc2;

  for (long i = threadIdx.x; i < len; i += blockDim.x)
    adamw_ex_element<S, SR>(p, g, m, v, i, start + i, ordinal, decay, step_size, inv_bc2, s);
}

// Grid-stride variant for tensors above the chunk table (see adamw.hip).
template <typename S, bool SR>
__global__ void adamw_single_ex_kernel(__hip_bfloat16* p, const __hip_bfloat16* __restrict__ g,
                                       S* m, S* v, long n, uint32_t ordinal,
                                       AdamWExScalars s) {
  const float decay = 1.f - s.lr * s.wd;
  const float step_size = s.lr / s.bc1;
  const float inv_bc2 = 1.f / s.bc2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    adamw_ex_element<S, SR>(p, g, m, v, i, i, ordinal, decay, step_size, inv_bc2, s);
}

static int single_grid_ex(long numel) {
  long blocks = (numel + 256 * 4 - 1) / (256 * 4);
  return (int)(blocks < 16384 ? blocks : 16384);
}

template <typename S, bool SR>
static void launch_adamw_ex(std::vector<torch::Tensor>& params, std::vector<torch::Tensor>& grads,
                            std::vector<torch::Tensor>& exp_avgs,
                            std::vector<torch::Tensor>& exp_avg_sqs,
                            const std::vector<int64_t>& ordinals, const AdamWExScalars& s,
                            hipStream_t stream) {
  size_t i = 0;
  while (i < params.size()) {
    const long numel0 = params[i].numel();
    if ((numel0 + MT_CHUNK - 1) / MT_CHUNK > MT_BLOCKS) {  // own full-chip launch
      hipLaunchKernelGGL((adamw_single_ex_kernel<S, SR>), dim3(single_grid_ex(numel0)),
                         dim3(256), 0, stream, (__hip_bfloat16*)params[i].data_ptr(),
                         (const __hip_bfloat16*)grads[i].data_ptr(),
                         (S*)exp_avgs[i].data_ptr(), (S*)exp_avg_sqs[i].data_ptr(), numel0,
                         (uint32_t)ordinals[i], s);
      HIP_CHECK_LAST();
      ++i;
      continue;
    }
    AdamWExArgs args;
    int nt = 0, nb = 0;
    while (i < params.size() && nt < MT_MAX) {
      const long numel = params[i].numel();
      const int chunks = (int)((numel + MT_CHUNK - 1) / MT_CHUNK);
      if (chunks > MT_BLOCKS || nb + chunks > MT_BLOCKS) break;
      args.p[nt] = params[i].data_ptr();
      args.g[nt] = grads[i].data_ptr();
      args.m[nt] = exp_avgs[i].data_ptr();
      args.v[nt] = exp_avg_sqs[i].data_ptr();
      args.numel[nt] = numel;
      args.ordinal[nt] = (uint32_t)ordinals[i];
      for (int c = 0; c < chunks; ++c) {
        args.tensor_of_block[nb] = (unsigned char)nt;
        args.chunk_of_block[nb] = c;
        ++nb;
      }
      ++nt;
      ++i;
    }
    if (nb == 0) {  // only empty tensors in this batch: nothing to launch
      if (nt == 0) break;
      continue;
    }
    hipLaunchKernelGGL((fused_adamw_ex_kernel<S, SR>), dim3(nb), dim3(256), 0, stream, args, s);
    HIP_CHECK_LAST();
  }
}

void fused_adamw_ex(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                    std::vector<torch::Tensor> exp_avgs, std::vector<torch::Tensor> exp_avg_sqs,
                    double lr, double beta1, double beta2, double eps, double wd, long step,
                    bool stochastic, int64_t seed, std::vector<int64_t> ordinals) {
  const size_t n = params.size();
  TORCH_CHECK(n == grads.size() && n == exp_avgs.size() && n == exp_avg_sqs.size() &&
                  n == ordinals.size(),
              "fused_adamw_ex: params, grads, moments and ordinals must have one entry per tensor");
  if (n == 0) return;
  const auto dev = params[0].device();
  TORCH_CHECK(dev.is_cuda(), "fused_adamw_ex: tensors must be on the GPU");
  const auto sdt = exp_avgs[0].scalar_type();
  TORCH_CHECK(sdt == torch::kBFloat16 || sdt == torch::kFloat32,
              "fused_adamw_ex: moments must be bfloat16 or float32");
  TORCH_CHECK(stochastic || sdt == torch::kFloat32,
              "fused_adamw_ex: bf16 moments with nearest rounding is the plain fused_adamw");
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(params[i].scalar_type() == torch::kBFloat16 &&
                    grads[i].scalar_type() == torch::kBFloat16,
                "fused_adamw_ex: parameters and grads must be bfloat16 (tensor ", i, ")");
    TORCH_CHECK(exp_avgs[i].scalar_type() == sdt && exp_avg_sqs[i].scalar_type() == sdt,
                "fused_adamw_ex: all moments in one call must share a dtype (tensor ", i, ")");
    TORCH_CHECK(params[i].device() == dev && grads[i].device() == dev &&
                    exp_avgs[i].device() == dev && exp_avg_sqs[i].device() == dev,
                "fused_adamw_ex: all tensors must be on the same device (tensor ", i, ")");
    TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous() &&
                    exp_avgs[i].is_contiguous() && exp_avg_sqs[i].is_contiguous(),
                "fused_adamw_ex: tensors must be contiguous (tensor ", i, ")");
    const long numel = params[i].numel();
    TORCH_CHECK(grads[i].numel() == numel && exp_avgs[i].numel() == numel &&
                    exp_avg_sqs[i].numel() == numel,
                "fused_adamw_ex: grad and moments must match the parameter's numel (tensor ", i, ")");
    TORCH_CHECK(ordinals[i] >= 0 && ordinals[i] <= 0xFFFFFFFFLL,
                "fused_adamw_ex: ordinal must fit in 32 bits (tensor ", i, ")");
  }
  TORCH_CHECK(step >= 1, "fused_adamw_ex: step must be >= 1");

  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  AdamWExScalars s;
  s.lr = (float)lr; s.beta1 = (float)beta1; s.beta2 = (float)beta2;
  s.eps = (float)eps; s.wd = (float)wd;
  s.bc1 = 1.f - powf((float)beta1, (float)step);
  s.bc2 = 1.f - powf((float)beta2, (float)step);
  s.seed_lo = (uint32_t)((uint64_t)seed);
  s.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  s.step = (uint32_t)step;

  if (sdt == torch::kBFloat16)
    launch_adamw_ex<__hip_bfloat16, true>(params, grads, exp_avgs, exp_avg_sqs, ordinals, s, stream);
  else if (stochastic)
    launch_adamw_ex<float, true>(params, grads, exp_avgs, exp_avg_sqs, ordinals, s, stream);
  else
    launch_adamw_ex<float, false>(params, grads, exp_avgs, exp_avg_sqs, ordinals, s, stream);
}

// ---------------------------------------------------------------------------
// stochastic_round_bf16: the rounding rule on its own (fp32 -> bf16)
// ---------------------------------------------------------------------------

__global__ void stochastic_round_kernel(const float* __restrict__ x, __hip_bfloat16* out, long n,
                                        uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                        uint32_t ordinal, int lane) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Philox4 r = philox_for_element(seed_lo, seed_hi, i, step, ordinal);
    out[i] = stochastic_round_bf16(x[i], philox_lane16(r, lane));
  }
}

torch::Tensor stochastic_round_bf16_op(torch::Tensor x, int64_t seed, long step, long ordinal,
                                       long lane) {
  TORCH_CHECK(x.is_cuda(), "stochastic_round_bf16: input must be on the GPU");
  TORCH_CHECK(x.scalar_type() == torch::kFloat32, "stochastic_round_bf16: input must be float32");
  TORCH_CHECK(x.is_contiguous(), "stochastic_round_bf16: input must be contiguous");
  TORCH_CHECK(lane >= 0 && lane <= 2, "stochastic_round_bf16: lane must be 0, 1 or 2");
  TORCH_CHECK(step >= 0 && step <= 0xFFFFFFFFL && ordinal >= 0 && ordinal <= 0xFFFFFFFFL,
              "stochastic_round_bf16: step and ordinal must fit in 32 bits");
  auto out = torch::empty_like(x, x.options().dtype(torch::kBFloat16));
  const long n = x.numel();
  if (n == 0) return out;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  hipLaunchKernelGGL(stochastic_round_kernel, dim3(single_grid_ex(n)), dim3(256), 0, stream,
                     x.data_ptr<float>(), (__hip_bfloat16*)out.data_ptr(), n,
                     (uint32_t)((uint64_t)seed), (uint32_t)((uint64_t)seed >> 32),
                     (uint32_t)step, (uint32_t)ordinal, (int)lane);
  HIP_CHECK_LAST();
  return out;
}
