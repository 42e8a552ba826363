#include "hip/hip_runtime.h"
// Per-head QK RMSNorm fused with RoPE (Qwen3 / OLMo-2 / Gemma-3 style
// attention-logit control): every (b, head, s) row x of head_dim elements of
// q and k goes through
//     invrms = rsqrt(mean(x^2) + eps)          fp32 sum and mean
//     n      = bf16(x * invrms)
//     y      = bf16(w * n)                     the two roundings of rmsnorm
//     out    = bf16(rope_rotate(y))            full rotary, position s
// in ONE pass over q and k (one 16-byte read and one write per element), where
// rmsnorm + rmsnorm + rope cost three.  The weight [hd] is shared by all
// heads of a tensor; q and k have their own.
//
// Addressing is rope_vec_kernel's: rows run in memory order ((b, s, h) for
// the transposed-BSHD view, (b, h, s) for BHSD), a lane owns one bf16x8 group
// of the first half of the row and its partner hd/2 further on.  A row is
// spread over LG adjacent lanes, LG the next power of two >= hd/16 (2, 4 or
// 8; lanes past hd/16 idle: hd 48 and 80), so the row sums are xor shuffles
// inside the lane group and the forward needs no LDS.  q's blocks come first,
// then k's: the choice of tensor is block-uniform.
//
// Backward, per row (g kept in fp32 throughout):
//     g  = rope_rotate<INVERSE>(dy)       nhat = x * invrms       dn = g * w
//     dx = bf16(invrms * (dn - nhat * mean(dn * nhat)))
//     dw_j = sum_rows g_j * nhat_j
// dw is deterministic: a capped grid strides over the row tiles, a lane
// accumulates its 16 columns in registers, a block reduces them through LDS
// once and writes one fp32 [hd] plane; qk_norm_dw_combine_kernel folds the
// planes in a fixed order.  No atomics.  The backward's tiles are rectangles
// of (heads x positions) of one batch entry, numbered and summed by (b, h, s)
// and not by address, so dw has the same bits for both layouts of a tensor;
// only which thread of the block takes which row of the tile follows memory.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"

namespace {

constexpr int QKN_BLOCK = 256;
// blocks per tensor in the backward: q and k together fill 256 CUs at 8 blocks
// each; the combine reads this many planes at most
constexpr int QKN_MAX_BLOCKS = 1024;
constexpr int QKN_COMBINE_BLOCK = 1024;

struct QknTensor {
  const __hip_bfloat16* x;   // input rows
  const __hip_bfloat16* dy;  // backward: gradient of the output, x's layout
  __hip_bfloat16* y;         // forward: output; backward: dx
  const __hip_bfloat16* w;   // [hd]
  float* invrms;             // [B, nh, S] contiguous; written fwd, read bwd
  float* part;               // backward: [blocks, hd] partial dw planes
  long bst, hst, ld;         // element strides of batch, head and position
  unsigned rows;             // B * nh * S
  unsigned tiles;            // row tiles of QKN_BLOCK / LG rows
  unsigned hblocks, sblocks; // backward: tiles per batch entry along h and s
  int hb;                    // backward: heads per tile, a power of two
  int blocks;                // blocks that work on this tensor
  int nh;
  int s_major;               // rows run (b, s, h): the transposed-BSHD view
};

struct QknArgs {
  QknTensor t[2];  // q, k
};

// memory-order row -> element offset of the row and index of its invrms
DEV_INLINE void qkn_row(const QknTensor& t, unsigned row, unsigned S, long& off,
                        long& stat, unsigned& s) {
  unsigned b, h;
  const unsigned nh = (unsigned)t.nh;
  if (t.s_major) {
    h = row % nh;
    s = (row / nh) % S;
    b = row / (nh * S);
  } else {
    s = row % S;
    h = (row / S) % nh;
    b = row / (S * nh);
  }
  off = b * t.bst + h * t.hst + s * t.ld;
  stat = ((long)b * nh + h) * S + s;
}

template <int LG>
DEV_INLINE float group_sum(float v) {
#pragma unroll
  for (int o = LG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;  // the same bits in every lane of the group
}

template <int LG>
__global__ __launch_bounds__(QKN_BLOCK) void qk_norm_rope_fwd_kernel(
    QknArgs a, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int S, int hd, float eps) {
  constexpr int RPB = QKN_BLOCK / LG;
  const int is_k = (int)blockIdx.x >= a.t[0].blocks;
  const QknTensor& t = a.t[is_k];
  const unsigned tile = is_k ? blockIdx.x - a.t[0].blocks : blockIdx.x;
  const int l = threadIdx.x % LG;
  const int half = hd / 2;
  const int i = l * 8;
  // a tile past 2^32 / RPB rows cannot exist: rows < 2^31 (host check)
  const unsigned row = tile * RPB + threadIdx.x / LG;
  const bool active = i < half && row < t.rows;

  long off = 0, stat = 0;
  unsigned s = 0;
  float x1[8], x2[8];
  // four chains, then the group's shuffles: at most 9 roundings on the way to
  // the row sum whatever hd is
  float ss[4] = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    qkn_row(t, row, (unsigned)S, off, stat, s);
    const Vec8<__hip_bfloat16> v1 = load8(t.x + off + i);
    const Vec8<__hip_bfloat16> v2 = load8(t.x + off + i + half);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x1[j] = to_f32(v1.v[j]);
      x2[j] = to_f32(v2.v[j]);
      ss[j & 1] = fmaf(x1[j], x1[j], ss[j & 1]);
      ss[2 + (j & 1)] = fmaf(x2[j], x2[j], ss[2 + (j & 1)]);
    }
  }
  const float sum = group_sum<LG>((ss[0] + ss[1]) + (ss[2] + ss[3]));
  if (!active) return;
  const float ir = rsqrtf(sum / hd + eps);
  if (l == 0) t.invrms[stat] = ir;

  const Vec8<__hip_bfloat16> w1 = load8(t.w + i);
  const Vec8<__hip_bfloat16> w2 = load8(t.w + i + half);
  const Vec8<float> c = load8(cos_t + (long)s * hd + i);
  const Vec8<float> sn = load8(sin_t + (long)s * hd + i);
  Vec8<__hip_bfloat16> o1, o2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // rmsnorm's roundings: (x * invrms) to bf16, then * w to bf16
    const __hip_bfloat16 n1 = from_f32<__hip_bfloat16>(x1[j] * ir);
    const __hip_bfloat16 n2 = from_f32<__hip_bfloat16>(x2[j] * ir);
    const __hip_bfloat16 y1 = from_f32<__hip_bfloat16>(to_f32(n1) * to_f32(w1.v[j]));
    const __hip_bfloat16 y2 = from_f32<__hip_bfloat16>(to_f32(n2) * to_f32(w2.v[j]));
    float r1, r2;
    rope_rotate<false>(to_f32(y1), to_f32(y2), c.v[j], sn.v[j], r1, r2);
    o1.v[j] = from_f32<__hip_bfloat16>(r1);
    o2.v[j] = from_f32<__hip_bfloat16>(r2);
  }
  store8(t.y + off + i, o1);
  store8(t.y + off + i + half, o2);
}

// 4 waves per SIMD: 128 VGPRs hold the 16 dw accumulators, the row's 32 fp32
// intermediates and the loads in flight without scratch
template <int LG>
__global__ __launch_bounds__(QKN_BLOCK, 4) void qk_norm_rope_bwd_kernel(
    QknArgs a, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int S, int hd) {
  constexpr int RPB = QKN_BLOCK / LG;
  // [RPB][hd] with hd <= 16 * LG
  __shared__ float red[QKN_BLOCK * 16];
  const int is_k = (int)blockIdx.x >= a.t[0].blocks;
  const QknTensor& t = a.t[is_k];
  const unsigned bl = is_k ? blockIdx.x - a.t[0].blocks : blockIdx.x;
  const int l = threadIdx.x % LG;
  const int half = hd / 2;
  const int i = l * 8;
  const bool lane_on = i < half;
  // a tile is hb heads x sb positions; the thread's row of it runs along
  // memory (h fastest in the transposed-BSHD view, s fastest in BHSD), its
  // slot in the reduction is h_loc * sb + s_loc whatever the layout
  const int sb = RPB / t.hb;
  const int rt = threadIdx.x / LG;
  const int h_loc = t.s_major ? rt % t.hb : rt / sb;
  const int s_loc = t.s_major ? rt / t.hb : rt % sb;
  const int r = h_loc * sb + s_loc;

  Vec8<__hip_bfloat16> w1, w2;
  if (lane_on) {
    w1 = load8(t.w + i);
    w2 = load8(t.w + i + half);
  }
  float acc1[8], acc2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc1[j] = acc2[j] = 0.f;

  // the trip count is block-uniform, so every lane reaches the shuffles
#pragma unroll 1
  for (unsigned tile = bl; tile < t.tiles; tile += (unsigned)t.blocks) {
    const unsigned s = (tile % t.sblocks) * sb + s_loc;
    const unsigned h = ((tile / t.sblocks) % t.hblocks) * t.hb + h_loc;
    const unsigned b = tile / (t.sblocks * t.hblocks);
    const bool active = lane_on && h < (unsigned)t.nh && s < (unsigned)S;
    long off = 0;
    float ir = 0.f, dot = 0.f;
    float dn1[8], dn2[8], n1[8], n2[8];
    if (active) {
      off = b * t.bst + h * t.hst + s * t.ld;
      ir = t.invrms[((long)b * t.nh + h) * S + s];
      const Vec8<__hip_bfloat16> xv1 = load8(t.x + off + i);
      const Vec8<__hip_bfloat16> xv2 = load8(t.x + off + i + half);
      const Vec8<__hip_bfloat16> dv1 = load8(t.dy + off + i);
      const Vec8<__hip_bfloat16> dv2 = load8(t.dy + off + i + half);
      const Vec8<float> c = load8(cos_t + (long)s * hd + i);
      const Vec8<float> sn = load8(sin_t + (long)s * hd + i);
      float d1 = 0.f, d2 = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g1, g2;
        rope_rotate<true>(to_f32(dv1.v[j]), to_f32(dv2.v[j]), c.v[j], sn.v[j], g1, g2);
        n1[j] = to_f32(xv1.v[j]) * ir;
        n2[j] = to_f32(xv2.v[j]) * ir;
        acc1[j] = fmaf(g1, n1[j], acc1[j]);
        acc2[j] = fmaf(g2, n2[j], acc2[j]);
        dn1[j] = g1 * to_f32(w1.v[j]);
        dn2[j] = g2 * to_f32(w2.v[j]);
        d1 = fmaf(dn1[j], n1[j], d1);
        d2 = fmaf(dn2[j], n2[j], d2);
      }
      dot = d1 + d2;
    }
    const float m = group_sum<LG>(dot) / hd;  // mean(dn * nhat)
    if (active) {
      Vec8<__hip_bfloat16> o1, o2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o1.v[j] = from_f32<__hip_bfloat16>(ir * (dn1[j] - n1[j] * m));
        o2.v[j] = from_f32<__hip_bfloat16>(ir * (dn2[j] - n2[j] * m));
      }
      store8(t.y + off + i, o1);
      store8(t.y + off + i + half, o2);
    }
  }

  if (lane_on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[r * hd + i + j] = acc1[j];
      red[r * hd + half + i + j] = acc2[j];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < hd) {
    float sum = 0.f;
    for (int rr = 0; rr < RPB; ++rr) sum += red[rr * hd + threadIdx.x];
    t.part[(long)bl * hd + threadIdx.x] = sum;
  }
}

// dw[col] = sum of the planes, in a fixed order: slice sl of a column adds
// planes sl, sl + SL, ..., then the SL slice sums are added in slice order.
// Block 0 folds q's planes, block 1 k's.
__global__ __launch_bounds__(QKN_COMBINE_BLOCK) void qk_norm_dw_combine_kernel(
    const float* __restrict__ part_q, int nq, const float* __restrict__ part_k, int nk,
    float* __restrict__ dwq, float* __restrict__ dwk, int hd, int hd_pad) {
  __shared__ float red[QKN_COMBINE_BLOCK];
  const float* part = blockIdx.x ? part_k : part_q;
  const int n = blockIdx.x ? nk : nq;
  float* out = blockIdx.x ? dwk : dwq;
  const int col = threadIdx.x % hd_pad;
  const int sl = threadIdx.x / hd_pad;
  const int SL = QKN_COMBINE_BLOCK / hd_pad;
  float sum = 0.f;
  if (col < hd)
    for (int p = sl; p < n; p += SL) sum += part[(long)p * hd + col];
  red[threadIdx.x] = sum;
  __syncthreads();
  if ((int)threadIdx.x < hd) {
    float tot = 0.f;
    for (int k = 0; k < SL; ++k) tot += red[k * hd_pad + threadIdx.x];
    out[threadIdx.x] = tot;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int lane_group(long hd) { return hd <= 32 ? 2 : (hd <= 64 ? 4 : 8); }

// rope_fwd's layout test
bool layout_ok(const torch::Tensor& q) {
  if (q.stride(3) != 1) return false;
  const long nh = q.size(1), S = q.size(2), hd = q.size(3);
  return q.is_contiguous() ||
         (q.stride(1) == hd && q.stride(2) == nh * hd && q.stride(0) == S * nh * hd);
}

// equal strides wherever a stride addresses anything
bool same_layout(const torch::Tensor& a, const torch::Tensor& b) {
  if (a.sizes() != b.sizes()) return false;
  for (int d = 0; d < a.dim(); ++d)
    if (a.size(d) > 1 && a.stride(d) != b.stride(d)) return false;
  return true;
}

void check_inputs(const char* op, const torch::Tensor& q, const torch::Tensor& k,
                  const torch::Tensor& wq, const torch::Tensor& wk,
                  const torch::Tensor& cos_t, const torch::Tensor& sin_t) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.scalar_type() == torch::kBFloat16 &&
              k.is_cuda() && k.dim() == 4 && k.scalar_type() == torch::kBFloat16 &&
              k.device() == q.device(),
              op, ": q and k must be 4-d bf16 tensors on one GPU");
  TORCH_CHECK(layout_ok(q) && layout_ok(k), op,
              ": q and k must each be BHSD-contiguous or the transposed view of a BSHD "
              "buffer");
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(2) == q.size(2) && k.size(3) == q.size(3),
              op, ": q and k must agree on batch, sequence and head_dim");
  const long hd = q.size(3);
  TORCH_CHECK(hd % 16 == 0 && hd >= 16 && hd <= 128, op,
              ": head_dim must be a multiple of 16 and at most 128, got ", hd);
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == hd, op,
              ": full rotary only, the tables must be [S_cache, head_dim]");
  TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda() && cos_t.device() == q.device() &&
              sin_t.device() == q.device() &&
              cos_t.scalar_type() == torch::kFloat32 &&
              sin_t.scalar_type() == torch::kFloat32 && cos_t.is_contiguous() &&
              sin_t.is_contiguous() && sin_t.sizes() == cos_t.sizes() &&
              cos_t.size(0) >= q.size(2),
              op, ": cos and sin must be fp32 contiguous tables of one shape with at "
              "least S rows");
  for (const torch::Tensor* w : {&wq, &wk})
    TORCH_CHECK(w->is_cuda() && w->device() == q.device() &&
                w->scalar_type() == torch::kBFloat16 && w->dim() == 1 &&
                w->size(0) == hd && w->is_contiguous(),
                op, ": the norm weights must be bf16 contiguous [head_dim]");
  bool vec_ok = aligned16(cos_t.data_ptr()) && aligned16(sin_t.data_ptr()) &&
                aligned16(wq.data_ptr()) && aligned16(wk.data_ptr());
  for (const torch::Tensor* x : {&q, &k})
    vec_ok = vec_ok && aligned16(x->data_ptr()) && x->stride(0) % 8 == 0 &&
             x->stride(1) % 8 == 0 && x->stride(2) % 8 == 0;
  TORCH_CHECK(vec_ok, op,
              ": pointers must be 16-byte aligned and strides multiples of 8 elements");
  TORCH_CHECK(q.size(0) * q.size(1) * q.size(2) < (1L << 31) &&
              k.size(0) * k.size(1) * k.size(2) < (1L << 31),
              op, ": more than 2^31 rows");
}

QknTensor make_tensor(const torch::Tensor& x, const torch::Tensor* dy, torch::Tensor& y,
                      const torch::Tensor& w, torch::Tensor& invrms, int lg, int max_blocks) {
  QknTensor t;
  t.x = (const __hip_bfloat16*)x.data_ptr();
  t.dy = dy ? (const __hip_bfloat16*)dy->data_ptr() : nullptr;
  t.y = (__hip_bfloat16*)y.data_ptr();
  t.w = (const __hip_bfloat16*)w.data_ptr();
  t.invrms = invrms.data_ptr<float>();
  t.part = nullptr;
  t.bst = x.stride(0);
  t.hst = x.stride(1);
  t.ld = x.stride(2);
  const long rows = x.size(0) * x.size(1) * x.size(2);
  const long rpb = QKN_BLOCK / lg;
  long tiles = (rows + rpb - 1) / rpb;
  t.hb = 1;
  t.hblocks = t.sblocks = 0;
  if (dy) {  // backward: (hb heads) x (rpb / hb positions) tiles, hb <= 4
    while (t.hb < 4 && t.hb * 2 <= x.size(1)) t.hb *= 2;
    const long sb = rpb / t.hb;
    t.hblocks = (unsigned)((x.size(1) + t.hb - 1) / t.hb);
    t.sblocks = (unsigned)((x.size(2) + sb - 1) / sb);
    tiles = x.size(0) * t.hblocks * t.sblocks;
  }
  t.rows = (unsigned)rows;
  t.tiles = (unsigned)tiles;
  t.blocks = (int)(max_blocks > 0 && tiles > max_blocks ? max_blocks : tiles);
  t.nh = (int)x.size(1);
  t.s_major = x.stride(1) < x.stride(2);
  return t;
}

}  // namespace

// (rows per block, block cap per tensor of the backward) for a head_dim: what
// decides how the dw reduction walks the rows
std::vector<int64_t> qk_norm_rope_geometry(int64_t hd) {
  return {QKN_BLOCK / lane_group(hd), QKN_MAX_BLOCKS};
}

std::vector<torch::Tensor> qk_norm_rope_fwd(torch::Tensor q, torch::Tensor k,
                                            torch::Tensor wq, torch::Tensor wk,
                                            torch::Tensor cos_t, torch::Tensor sin_t,
                                            double eps) {
  check_inputs("qk_norm_rope_fwd", q, k, wq, wk, cos_t, sin_t);
  TORCH_CHECK(eps >= 0, "qk_norm_rope_fwd: eps must be >= 0, got ", eps);
  const int S = q.size(2), hd = q.size(3);
  auto qo = torch::empty_strided(q.sizes(), q.strides(), q.options());
  auto ko = torch::empty_strided(k.sizes(), k.strides(), k.options());
  auto fopt = q.options().dtype(torch::kFloat32);
  auto iq = torch::empty({q.size(0), q.size(1), q.size(2)}, fopt);
  auto ik = torch::empty({k.size(0), k.size(1), k.size(2)}, fopt);
  const int lg = lane_group(hd);
  QknArgs a;
  a.t[0] = make_tensor(q, nullptr, qo, wq, iq, lg, 0);
  a.t[1] = make_tensor(k, nullptr, ko, wk, ik, lg, 0);
  const long nblocks = (long)a.t[0].blocks + a.t[1].blocks;
  if (nblocks == 0) return {qo, ko, iq, ik};
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid(nblocks), block(QKN_BLOCK);
  const float* c = cos_t.data_ptr<float>();
  const float* s = sin_t.data_ptr<float>();
  if (lg == 2)
    hipLaunchKernelGGL(qk_norm_rope_fwd_kernel<2>, grid, block, 0, stream, a, c, s, S, hd,
                       (float)eps);
  else if (lg == 4)
    hipLaunchKernelGGL(qk_norm_rope_fwd_kernel<4>, grid, block, 0, stream, a, c, s, S, hd,
                       (float)eps);
  else
    hipLaunchKernelGGL(qk_norm_rope_fwd_kernel<8>, grid, block, 0, stream, a, c, s, S, hd,
                       (float)eps);
  HIP_CHECK_LAST();
  return {qo, ko, iq, ik};
}

std::vector<torch::Tensor> qk_norm_rope_bwd(torch::Tensor dqo, torch::Tensor dko,
                                            torch::Tensor q, torch::Tensor k,
                                            torch::Tensor wq, torch::Tensor wk,
                                            torch::Tensor invrms_q, torch::Tensor invrms_k,
                                            torch::Tensor cos_t, torch::Tensor sin_t) {
  check_inputs("qk_norm_rope_bwd", q, k, wq, wk, cos_t, sin_t);
  for (int i = 0; i < 2; ++i) {
    const torch::Tensor& x = i ? k : q;
    const torch::Tensor& ir = i ? invrms_k : invrms_q;
    const torch::Tensor& dy = i ? dko : dqo;
    TORCH_CHECK(ir.is_cuda() && ir.device() == x.device() &&
                ir.scalar_type() == torch::kFloat32 && ir.is_contiguous() &&
                ir.dim() == 3 && ir.size(0) == x.size(0) && ir.size(1) == x.size(1) &&
                ir.size(2) == x.size(2),
                "qk_norm_rope_bwd: invrms must be fp32 contiguous [B, heads, S]");
    TORCH_CHECK(dy.is_cuda() && dy.device() == x.device() &&
                dy.scalar_type() == torch::kBFloat16 && same_layout(dy, x) &&
                aligned16(dy.data_ptr()),
                "qk_norm_rope_bwd: the output gradients must be bf16 in the layout of q "
                "and k, 16-byte aligned");
  }
  const int S = q.size(2), hd = q.size(3);
  auto dq = torch::empty_strided(q.sizes(), q.strides(), q.options());
  auto dk = torch::empty_strided(k.sizes(), k.strides(), k.options());
  auto fopt = q.options().dtype(torch::kFloat32);
  const int lg = lane_group(hd);
  QknArgs a;
  a.t[0] = make_tensor(q, &dqo, dq, wq, invrms_q, lg, QKN_MAX_BLOCKS);
  a.t[1] = make_tensor(k, &dko, dk, wk, invrms_k, lg, QKN_MAX_BLOCKS);
  auto part_q = torch::empty({a.t[0].blocks, hd}, fopt);
  auto part_k = torch::empty({a.t[1].blocks, hd}, fopt);
  a.t[0].part = part_q.data_ptr<float>();
  a.t[1].part = part_k.data_ptr<float>();
  auto dw = torch::empty({2, hd}, fopt);
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const long nblocks = (long)a.t[0].blocks + a.t[1].blocks;
  const float* c = cos_t.data_ptr<float>();
  const float* s = sin_t.data_ptr<float>();
  if (nblocks > 0) {
    dim3 grid(nblocks), block(QKN_BLOCK);
    if (lg == 2)
      hipLaunchKernelGGL(qk_norm_rope_bwd_kernel<2>, grid, block, 0, stream, a, c, s, S, hd);
    else if (lg == 4)
      hipLaunchKernelGGL(qk_norm_rope_bwd_kernel<4>, grid, block, 0, stream, a, c, s, S, hd);
    else
      hipLaunchKernelGGL(qk_norm_rope_bwd_kernel<8>, grid, block, 0, stream, a, c, s, S, hd);
  }
  const int hd_pad = 16 * lg;
  hipLaunchKernelGGL(qk_norm_dw_combine_kernel, dim3(2), dim3(QKN_COMBINE_BLOCK), 0, stream,
                     part_q.data_ptr<float>(), a.t[0].blocks, part_k.data_ptr<float>(),
                     a.t[1].blocks, dw.data_ptr<float>(), dw.data_ptr<float>() + hd, hd,
                     hd_pad);
  HIP_CHECK_LAST();
  return {dq, dk, dw[0], dw[1]};
}
