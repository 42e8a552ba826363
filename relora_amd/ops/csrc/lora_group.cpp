// Group LoRA linear: forward and backward for G <= 3 sibling projections
// that share one input (q/k/v, gate/up).  Does for the group what
// _FusedLoRALinear (ops/functional.py) does for one linear, but
//   * dropout + the rank-r down-projection of ALL siblings is one
//     lora_down_dropout launch that reads x once and writes no dropped copy;
//   * backward accumulates every sibling's input gradient (main and LoRA
//     part) into ONE dx buffer: GEMM beta=1 for the main parts, lora_add_nn_
//     (already an accumulate) for the LoRA parts — no per-sibling dx, no
//     autograd fork adds, no mask_apply pass.
// The main GEMMs stay on the library (or fused_lora_gemm where the caller's
// per-sibling flag says the single-linear path would pick it).

#include <torch/extension.h>

std::vector<torch::Tensor> lora_down_dropout(torch::Tensor x, std::vector<torch::Tensor> As,
                                             std::vector<int64_t> seeds, double p);
void lora_add_nt_(torch::Tensor out, torch::Tensor P, torch::Tensor Q);
void lora_add_nt_rope_group_(std::vector<torch::Tensor> outs, std::vector<torch::Tensor> Ps,
                             std::vector<torch::Tensor> Qs, std::vector<int64_t> rotary,
                             torch::Tensor cos_t, torch::Tensor sin_t, int64_t S, int64_t hd);
void lora_add_nn_(torch::Tensor out, torch::Tensor P, torch::Tensor Q,
                  torch::Tensor mask, double inv_keep);
torch::Tensor fused_lora_gemm(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                              torch::Tensor bw, torch::Tensor bias, double lora_scale);
torch::Tensor skinny_grad(torch::Tensor P, torch::Tensor X, torch::Tensor xmask,
                          double inv_keep, double scale,
                          bool transpose_out, torch::ScalarType dtype);
void lora_add_nn_group_(torch::Tensor out, std::vector<torch::Tensor> Ps,
                        std::vector<torch::Tensor> Qs, std::vector<torch::Tensor> masks,
                        double inv_keep);
std::vector<torch::Tensor> skinny_grad_group(std::vector<torch::Tensor> Ps, torch::Tensor X,
                                             std::vector<torch::Tensor> masks,
                                             double inv_keep, torch::ScalarType dtype);

// x[M,K]; per sibling g: W_g[N_g,K], bias_g ([N_g] or empty), A_g[r,K],
// B_g[N_g,r], scale_g, seed_g, fused_g (use fused_lora_gemm for this one).
// Returns 4 tensors per sibling, grouped: {y_0..}, {t_0..}, {bs_0..},
// {mask_0..} (masks only when p > 0), with bs_g = scale_g * B_g.
//
// With cos/sin given (fp32 [S_cache, hd] tables; x is [B*S, K], row m sits at
// position m % S), the siblings flagged in `rotary` come back RoPE-rotated:
// the G lora_add_nt_ launches and the separate rope pass become one
// lora_add_nt_rope_group_ launch.  The caller asks for this only where that
// kernel's constraints hold (ops/functional.py: lora_group_rope_ok); anything
// else is an error here, not a fall-back.
std::vector<torch::Tensor> lora_group_fwd(
    torch::Tensor x, std::vector<torch::Tensor> Ws, std::vector<torch::Tensor> biases,
    std::vector<torch::Tensor> As, std::vector<torch::Tensor> Bs,
    std::vector<double> scales, std::vector<int64_t> seeds, double p,
    std::vector<int64_t> fused, c10::optional<torch::Tensor> cos_t,
    c10::optional<torch::Tensor> sin_t, std::vector<int64_t> rotary, int64_t S,
    int64_t hd) {
  const size_t G = Ws.size();
  TORCH_CHECK(G >= 1 && G <= 3 && biases.size() == G && As.size() == G &&
              Bs.size() == G && scales.size() == G && fused.size() == G,
              "lora_group_fwd: per-sibling lists must have 1..3 entries each");
  const bool rope = cos_t.has_value();
  if (rope) {
    TORCH_CHECK(sin_t.has_value() && rotary.size() == G,
                "lora_group_fwd: rope needs cos, sin and one rotary flag per sibling");
    for (size_t g = 0; g < G; ++g)
      TORCH_CHECK(!fused[g], "lora_group_fwd: rope cannot follow fused_lora_gemm siblings");
  }
  auto tm = lora_down_dropout(x, As, seeds, p);  // {t_0.., mask_0..}
  std::vector<torch::Tensor> ys, bss;
  for (size_t g = 0; g < G; ++g) {
    const auto& t = tm[g];
    const bool has_bias = biases[g].defined() && biases[g].numel() > 0;
    auto bs = Bs[g] * scales[g];
    const int64_t N = Ws[g].size(0);
    torch::Tensor y;
    if (fused[g]) {
      y = fused_lora_gemm(x, Ws[g], t, Bs[g],
                          has_bias ? biases[g] : x.new_empty({0}), scales[g]);
    } else {
      y = has_bias ? at::linear(x, Ws[g], biases[g]) : at::linear(x, Ws[g]);
      if (rope) {
        // added (and rotated) below, all siblings in one launch
      } else if (N % 8 == 0) {
        lora_add_nt_(y, t, bs);                  // y += t @ bs^T
      } else {
        y.addmm_(t, bs.t());                     // library, beta = 1
      }
    }
    ys.push_back(y);
    bss.push_back(bs);
  }
  if (rope) {
    std::vector<torch::Tensor> ts(tm.begin(), tm.begin() + G);
    lora_add_nt_rope_group_(ys, ts, bss, rotary, *cos_t, *sin_t, S, hd);
  }
  std::vector<torch::Tensor> out(ys);
  out.insert(out.end(), tm.begin(), tm.begin() + G);
  out.insert(out.end(), bss.begin(), bss.end());
  out.insert(out.end(), tm.begin() + G, tm.end());
  return out;
}

// dys[g]: [M,N_g] contiguous.  masks empty (size 0 list) when p == 0.
// Returns {dx, dA_0.., dB_0..}.
// group_bwd (RELORA_AMD_LORA_GROUP_BWD): with G >= 2, the LoRA parts of dx go
// into dx in one lora_add_nn_group_ pass (one read-modify-write of dx, one
// rounding) and every dA_g comes from one skinny_grad_group launch (x read
// once).  Off: one lora_add_nn_ and one skinny_grad per sibling.
std::vector<torch::Tensor> lora_group_bwd(
    std::vector<torch::Tensor> dys, torch::Tensor x, std::vector<torch::Tensor> masks,
    std::vector<torch::Tensor> ts, std::vector<torch::Tensor> Ws,
    std::vector<torch::Tensor> As, std::vector<torch::Tensor> bss,
    std::vector<double> scales, double p, bool group_bwd) {
  const size_t G = dys.size();
  TORCH_CHECK(G >= 1 && G <= 3 && ts.size() == G && Ws.size() == G && As.size() == G &&
              bss.size() == G && scales.size() == G,
              "lora_group_bwd: per-sibling lists must have 1..3 entries each");
  const bool drop = p > 0.0;
  TORCH_CHECK(!drop || masks.size() == G, "lora_group_bwd: one mask per sibling");
  const double inv_keep = drop ? 1.0 / (1.0 - p) : 1.0;
  auto empty_mask = x.new_empty({0}, x.options().dtype(torch::kUInt8));

  // one dx for the whole group: first sibling writes, the rest accumulate
  auto dx = at::mm(dys[0], Ws[0]);
  for (size_t g = 1; g < G; ++g) dx.addmm_(dys[g], Ws[g]);

  const bool fuse = group_bwd && G >= 2;
  std::vector<torch::Tensor> us, dAs, dBs;
  for (size_t g = 0; g < G; ++g) {
    const auto& mask = drop ? masks[g] : empty_mask;
    auto u = at::mm(dys[g], bss[g]);             // [M, r] = s * dy @ B
    if (fuse) {
      us.push_back(u);
    } else {
      lora_add_nn_(dx, u, As[g], mask, inv_keep);  // dx += mask/(1-p) * (u @ A)
      dAs.push_back(skinny_grad(u, x, mask, inv_keep, 1.0, false, As[g].scalar_type()));
    }
    const int64_t N = Ws[g].size(0);
    if (N % 8 == 0) {
      dBs.push_back(skinny_grad(ts[g], dys[g], empty_mask, 1.0, scales[g], true,
                                bss[g].scalar_type()));
    } else {
      dBs.push_back(at::mm(dys[g].t(), ts[g]) * scales[g]);
    }
  }
  if (fuse) {
    if (!drop) masks.clear();
    lora_add_nn_group_(dx, us, As, masks, inv_keep);  // dx += sum_g mask_g/(1-p) * (u_g @ A_g)
    dAs = skinny_grad_group(us, x, masks, inv_keep, As[0].scalar_type());
  }
  std::vector<torch::Tensor> out{dx};
  out.insert(out.end(), dAs.begin(), dAs.end());
  out.insert(out.end(), dBs.begin(), dBs.end());
  return out;
}
