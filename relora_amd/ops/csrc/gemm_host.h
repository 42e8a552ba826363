// Host preparation shared by the fused GEMM entry points (fused_gemm.hip,
// fp8_gemm.hip, mxfp4_gemm.hip): the LoRA and bias arguments.  The kernels
// index t, bw and bias from M, N and r alone, so whatever is not checked here
// is read out of bounds on a mismatch.  `anchor` names the tensor whose device
// `dev` is ("x", or "xq" for the one-byte kernels) in the messages.
#pragma once

#include <hip/hip_bf16.h>
#include <torch/extension.h>

struct LoraArgs {
  int r = 0;               // 0 without LoRA
  torch::Tensor t_scaled;  // keeps the folded t alive until the launch
  const __hip_bfloat16* t = nullptr;
  const __hip_bfloat16* bw = nullptr;
  const __hip_bfloat16* bias = nullptr;
};

static inline void check_bf16_arg(const char* fn, const char* what, const torch::Tensor& v,
                                  const torch::Device& dev, const char* anchor) {
  TORCH_CHECK(v.device() == dev, fn, ": ", what, " must be on ", anchor, "'s device");
  TORCH_CHECK(v.scalar_type() == torch::kBFloat16, fn, ": ", what, " must be bf16");
  TORCH_CHECK(v.is_contiguous(), fn, ": ", what, " must be contiguous");
}

// All checks run before the lora_scale == 1.0 shortcut that hands `t` to the
// kernel as it came.
static inline LoraArgs prep_lora_bias(const char* fn, const char* anchor, const torch::Device& dev,
                                      const torch::Tensor& t, const torch::Tensor& bw,
                                      const torch::Tensor& bias, long M, long N, int r_step,
                                      int r_max, double lora_scale) {
  LoraArgs a;
  const bool has_lora = t.defined() && t.numel() > 0;
  if (has_lora) {
    check_bf16_arg(fn, "t", t, dev, anchor);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == M, fn, ": t must be [M, r]");
    const long r = t.size(1);
    TORCH_CHECK(r % r_step == 0 && r <= r_max, fn, ": r must be a multiple of ", r_step,
                ", <= ", r_max);
    TORCH_CHECK(bw.defined(), fn, ": bw is required with t");
    check_bf16_arg(fn, "bw", bw, dev, anchor);
    TORCH_CHECK(bw.dim() == 2 && bw.size(0) == N && bw.size(1) == r, fn, ": bw must be [N, r]");
    a.r = (int)r;
  }
  if (bias.defined() && bias.numel() > 0) {
    check_bf16_arg(fn, "bias", bias, dev, anchor);
    TORCH_CHECK(bias.numel() == N, fn, ": bias must have N elements");
    a.bias = (const __hip_bfloat16*)bias.data_ptr();
  }
  if (a.r > 0) {
    // fold the LoRA scale into t (bf16 rounding of s*t matches the composed
    // path, which also rounds t·B^T·s contributions in bf16)
    a.t_scaled = (lora_scale == 1.0) ? t : (t * lora_scale).contiguous();
    a.t = (const __hip_bfloat16*)a.t_scaled.data_ptr();
    a.bw = (const __hip_bfloat16*)bw.data_ptr();
  }
  return a;
}
