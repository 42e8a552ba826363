// Python bindings for the relora_amd gfx950 HIP kernels.

#include <torch/extension.h>

// norms.hip
std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps);
std::vector<torch::Tensor> rmsnorm_fwd_add(torch::Tensor x, torch::Tensor res,
                                           torch::Tensor w, double eps);
std::vector<torch::Tensor> rmsnorm_bwd_add(torch::Tensor x, torch::Tensor w,
                                           torch::Tensor invrms, torch::Tensor dy,
                                           torch::Tensor dsum);
std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor x, torch::Tensor w,
                                       torch::Tensor invrms, torch::Tensor dy);
std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps);
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor mean, torch::Tensor invstd,
                                         torch::Tensor dy);
// rope.hip
std::vector<torch::Tensor> rope_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor cos_t, torch::Tensor sin_t,
                                    bool inverse, bool force_scalar);
// qk_norm_rope.hip
std::vector<torch::Tensor> qk_norm_rope_fwd(torch::Tensor q, torch::Tensor k,
                                            torch::Tensor wq, torch::Tensor wk,
                                            torch::Tensor cos_t, torch::Tensor sin_t,
                                            double eps);
std::vector<torch::Tensor> qk_norm_rope_bwd(torch::Tensor dqo, torch::Tensor dko,
                                            torch::Tensor q, torch::Tensor k,
                                            torch::Tensor wq, torch::Tensor wk,
                                            torch::Tensor invrms_q, torch::Tensor invrms_k,
                                            torch::Tensor cos_t, torch::Tensor sin_t);
std::vector<int64_t> qk_norm_rope_geometry(int64_t hd);
// swiglu.hip
torch::Tensor swiglu_fwd(torch::Tensor g, torch::Tensor u);
torch::Tensor gelu_fwd(torch::Tensor x);
torch::Tensor gelu_bwd(torch::Tensor x, torch::Tensor dy);
std::vector<torch::Tensor> swiglu_bwd(torch::Tensor g, torch::Tensor u, torch::Tensor dy);
// ce.hip
std::vector<torch::Tensor> ce_row_stats(torch::Tensor logits, torch::Tensor labels,
                                        long ignore_index);
void ce_grad_(torch::Tensor logits, torch::Tensor labels, torch::Tensor lse,
              double gscale, long ignore_index);
std::vector<torch::Tensor> ce_row_stats_ex(torch::Tensor logits, torch::Tensor labels,
                                           long ignore_index);
void ce_grad_ex_(torch::Tensor logits, torch::Tensor labels, torch::Tensor lse,
                 double gscale, double z_loss, double label_smoothing, long ignore_index);
// adamw.hip
void fused_adamw(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                 std::vector<torch::Tensor> exp_avgs, std::vector<torch::Tensor> exp_avg_sqs,
                 double lr, double beta1, double beta2, double eps, double wd, long step);
torch::Tensor multi_tensor_l2norm(std::vector<torch::Tensor> grads);
void multi_tensor_scale_(std::vector<torch::Tensor> grads, double scale);
// adamw_ex.hip
void fused_adamw_ex(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
                    std::vector<torch::Tensor> exp_avgs, std::vector<torch::Tensor> exp_avg_sqs,
                    double lr, double beta1, double beta2, double eps, double wd, long step,
                    bool stochastic, int64_t seed, std::vector<int64_t> ordinals);
torch::Tensor stochastic_round_bf16_op(torch::Tensor x, int64_t seed, long step, long ordinal,
                                       long lane);
// lora_gemm.hip
std::vector<torch::Tensor> dropout_mask_fwd(torch::Tensor x, double p, int64_t seed);
torch::Tensor dropout_mask_bwd(torch::Tensor dy, torch::Tensor mask, double p);
void lora_add_nt_(torch::Tensor out, torch::Tensor P, torch::Tensor Q);
void lora_add_nt_rope_group_(std::vector<torch::Tensor> outs, std::vector<torch::Tensor> Ps,
                             std::vector<torch::Tensor> Qs, std::vector<int64_t> rotary,
                             torch::Tensor cos_t, torch::Tensor sin_t, int64_t S, int64_t hd);
std::vector<torch::Tensor> lora_down_dropout(torch::Tensor x, std::vector<torch::Tensor> As,
                                             std::vector<int64_t> seeds, double p);
// lora_group.cpp
std::vector<torch::Tensor> lora_group_fwd(
    torch::Tensor x, std::vector<torch::Tensor> Ws, std::vector<torch::Tensor> biases,
    std::vector<torch::Tensor> As, std::vector<torch::Tensor> Bs,
    std::vector<double> scales, std::vector<int64_t> seeds, double p,
    std::vector<int64_t> fused, c10::optional<torch::Tensor> cos_t,
    c10::optional<torch::Tensor> sin_t, std::vector<int64_t> rotary, int64_t S,
    int64_t hd);
std::vector<torch::Tensor> lora_group_bwd(
    std::vector<torch::Tensor> dys, torch::Tensor x, std::vector<torch::Tensor> masks,
    std::vector<torch::Tensor> ts, std::vector<torch::Tensor> Ws,
    std::vector<torch::Tensor> As, std::vector<torch::Tensor> bss,
    std::vector<double> scales, double p, bool group_bwd);

// fused_gemm.hip
torch::Tensor fused_lora_gemm(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                              torch::Tensor bw, torch::Tensor bias, double lora_scale);
torch::Tensor fused_lora_gemm3(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                               torch::Tensor bw, torch::Tensor bias, double lora_scale);
torch::Tensor fused_lora_gemm4(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                               torch::Tensor bw, torch::Tensor bias, double lora_scale);
torch::Tensor fused_int8_gemm(torch::Tensor x, torch::Tensor qw, torch::Tensor amax,
                              long N, torch::Tensor t, torch::Tensor bw,
                              torch::Tensor bias, double lora_scale);
torch::Tensor fused_nf4_gemm(torch::Tensor x, torch::Tensor qw, torch::Tensor amax,
                             long N, torch::Tensor t, torch::Tensor bw,
                             torch::Tensor bias, double lora_scale);
void lora_add_nn_(torch::Tensor out, torch::Tensor P, torch::Tensor Q,
                  torch::Tensor mask, double inv_keep);
torch::Tensor skinny_grad(torch::Tensor P, torch::Tensor X, torch::Tensor xmask,
                          double inv_keep, double scale,
                          bool transpose_out, torch::ScalarType dtype);
void lora_add_nn_group_(torch::Tensor out, std::vector<torch::Tensor> Ps,
                        std::vector<torch::Tensor> Qs, std::vector<torch::Tensor> masks,
                        double inv_keep);
std::vector<torch::Tensor> skinny_grad_group(std::vector<torch::Tensor> Ps, torch::Tensor X,
                                             std::vector<torch::Tensor> masks,
                                             double inv_keep, torch::ScalarType dtype);
// quantize.hip
std::vector<torch::Tensor> quantize_nf4(torch::Tensor x);
torch::Tensor dequantize_nf4(torch::Tensor q, torch::Tensor absmax, long n, torch::ScalarType dtype);
std::vector<torch::Tensor> quantize_int8(torch::Tensor x);
torch::Tensor dequantize_int8(torch::Tensor q, torch::Tensor absmax, long n, torch::ScalarType dtype);
// attention.hip
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    double scale, c10::optional<torch::Tensor> doc_start);
std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse, torch::Tensor dout,
                                    double scale, c10::optional<torch::Tensor> doc_start);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd, "RMSNorm forward (gfx950)");
  m.def("rmsnorm_bwd", &rmsnorm_bwd, "RMSNorm backward (gfx950)");
  m.def("rmsnorm_fwd_add", &rmsnorm_fwd_add, "fused residual-add + RMSNorm fwd (gfx950)");
  m.def("rmsnorm_bwd_add", &rmsnorm_bwd_add, "RMSNorm bwd with +dsum fused into dx (gfx950)");
  m.def("layernorm_fwd", &layernorm_fwd, "LayerNorm forward (gfx950)");
  m.def("layernorm_bwd", &layernorm_bwd, "LayerNorm backward (gfx950)");
  // force_scalar: run the one-pair-per-thread kernel where the vectorised one
  // would be taken (the tests compare the two)
  m.def("rope_fwd", &rope_fwd, "RoPE apply fwd/inverse (gfx950)",
        py::arg("q"), py::arg("k"), py::arg("cos"), py::arg("sin"), py::arg("inverse"),
        py::arg("force_scalar") = false);
  m.def("qk_norm_rope_fwd", &qk_norm_rope_fwd,
        "per-head RMSNorm of q and k fused with RoPE, one launch (gfx950)",
        py::arg("q"), py::arg("k"), py::arg("wq"), py::arg("wk"), py::arg("cos"),
        py::arg("sin"), py::arg("eps"));
  m.def("qk_norm_rope_bwd", &qk_norm_rope_bwd,
        "backward of qk_norm_rope_fwd: dq, dk and the fp32 weight gradients (gfx950)",
        py::arg("dqo"), py::arg("dko"), py::arg("q"), py::arg("k"), py::arg("wq"),
        py::arg("wk"), py::arg("invrms_q"), py::arg("invrms_k"), py::arg("cos"),
        py::arg("sin"));
  m.def("qk_norm_rope_geometry", &qk_norm_rope_geometry,
        "(rows per block, backward block cap per tensor) of qk_norm_rope for a head_dim");
  m.def("swiglu_fwd", &swiglu_fwd, "SwiGLU forward (gfx950)");
  m.def("swiglu_bwd", &swiglu_bwd, "SwiGLU backward (gfx950)");
  m.def("gelu_fwd", &gelu_fwd, "exact-erf GELU forward (gfx950)");
  m.def("gelu_bwd", &gelu_bwd, "exact-erf GELU backward (gfx950)");
  m.def("ce_row_stats", &ce_row_stats, "CE row lse/target (gfx950)");
  m.def("ce_grad_", &ce_grad_, "CE in-place softmax-onehot grad (gfx950)");
  m.def("ce_row_stats_ex", &ce_row_stats_ex, "CE row lse/target/row-sum (gfx950)");
  m.def("ce_grad_ex_", &ce_grad_ex_,
        "CE in-place grad with z-loss and label smoothing (gfx950)");
  m.def("fused_adamw", &fused_adamw, "multi-tensor AdamW step (gfx950)");
  m.def("fused_adamw_ex", &fused_adamw_ex,
        "multi-tensor AdamW step, bf16 params with fp32 moments and/or stochastic rounding "
        "(gfx950)",
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"), py::arg("exp_avg_sqs"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("wd"),
        py::arg("step"), py::arg("stochastic"), py::arg("seed"), py::arg("ordinals"));
  m.def("stochastic_round_bf16", &stochastic_round_bf16_op,
        "fp32 -> bf16 stochastic rounding with Philox4x32-10 bits (gfx950)",
        py::arg("x"), py::arg("seed"), py::arg("step"), py::arg("ordinal"), py::arg("lane"));
  m.def("multi_tensor_l2norm", &multi_tensor_l2norm, "multi-tensor L2 norm (gfx950)");
  m.def("multi_tensor_scale_", &multi_tensor_scale_, "multi-tensor scale (gfx950)");
  m.def("dropout_mask_fwd", &dropout_mask_fwd, "fused dropout + packed mask (gfx950)");
  m.def("dropout_mask_bwd", &dropout_mask_bwd, "packed-mask dropout backward (gfx950)");
  m.def("lora_add_nt_", &lora_add_nt_, "out += P @ Q^T rank-r MFMA accumulate (gfx950)");
  m.def("lora_down_dropout", &lora_down_dropout,
        "t_g = dropout_g(x) @ A_g^T for up to 3 siblings, x read once (gfx950)");
  m.def("lora_add_nt_rope_group_", &lora_add_nt_rope_group_,
        "out_g += P_g @ Q_g^T for 1..3 siblings in one launch, RoPE applied in place to "
        "the flagged ones (gfx950)",
        py::arg("outs"), py::arg("Ps"), py::arg("Qs"), py::arg("rotary"), py::arg("cos"),
        py::arg("sin"), py::arg("S"), py::arg("hd"));
  // cos/sin/rotary/S/hd: rotate the flagged siblings in the LoRA epilogue
  m.def("lora_group_fwd", &lora_group_fwd,
        "group LoRA linear forward for siblings sharing one input (gfx950)",
        py::arg("x"), py::arg("Ws"), py::arg("biases"), py::arg("As"), py::arg("Bs"),
        py::arg("scales"), py::arg("seeds"), py::arg("p"), py::arg("fused"),
        py::arg("cos") = py::none(), py::arg("sin") = py::none(),
        py::arg("rotary") = std::vector<int64_t>(), py::arg("S") = 0, py::arg("hd") = 0);
  m.def("lora_group_bwd", &lora_group_bwd,
        "group LoRA linear backward into one shared dx (gfx950)",
        py::arg("dys"), py::arg("x"), py::arg("masks"), py::arg("ts"), py::arg("Ws"),
        py::arg("As"), py::arg("bss"), py::arg("scales"), py::arg("p"),
        py::arg("group_bwd") = true);
  m.def("fused_lora_gemm", &fused_lora_gemm,
        "y = x@W^T (+bias) + s*t@Bw^T fused MFMA GEMM, 256^2 glds tile (gfx950)");
  m.def("fused_lora_gemm3", &fused_lora_gemm3,
        "3-buffer counted-vmcnt deep-pipelined fused GEMM variant (gfx950)");
  m.def("fused_lora_gemm4", &fused_lora_gemm4,
        "BK=32 4-buffer counted-vmcnt fused GEMM (glds-span tier, gfx950)");
  m.def("fused_int8_gemm", &fused_int8_gemm,
        "y = x@dequant_int8(W)^T + s*t@Bw^T, dequant fused into staging (gfx950)");
  m.def("fused_nf4_gemm", &fused_nf4_gemm,
        "y = x@dequant(W)^T + s*t@Bw^T with NF4 dequant fused into LDS staging (gfx950)");
  m.def("lora_add_nn_", &lora_add_nn_, "out += maskscale*(P @ Q) rank-r MFMA accumulate (gfx950)");
  m.def("skinny_grad", &skinny_grad, "P^T @ X chunked fp32 reduction (gfx950)");
  m.def("lora_add_nn_group_", &lora_add_nn_group_,
        "out += sum_g maskscale_g*(P_g @ Q_g), one pass over out for 1..3 siblings (gfx950)");
  m.def("skinny_grad_group", &skinny_grad_group,
        "P_g^T @ mask_g(X) for 1..3 siblings, X read once (gfx950)");
  m.def("quantize_nf4", &quantize_nf4, "NF4 blockwise quantize (gfx950)");
  m.def("dequantize_nf4", &dequantize_nf4, "NF4 blockwise dequantize (gfx950)");
  m.def("quantize_int8", &quantize_int8, "int8 blockwise quantize (gfx950)");
  m.def("dequantize_int8", &dequantize_int8, "int8 blockwise dequantize (gfx950)");
  // doc_start: optional int32 [B, S] intra-document mask (padded head_dim <= 64)
  m.def("attn_fwd", &attn_fwd, "causal flash attention forward (gfx950 MFMA)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("doc_start") = py::none());
  m.def("attn_bwd", &attn_bwd, "causal flash attention backward (gfx950 MFMA)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"),
        py::arg("dout"), py::arg("scale"), py::arg("doc_start") = py::none());
}
