#include "hip/hip_runtime.h"
// Fused LoRA rank-r update kernels (K1+K2) for gfx950.
//
// The reference computes the LoRA path as three separate torch ops plus an
// add (reference relora.py:319-323): dropout(x), lora_A GEMM, lora_B GEMM,
// scale-mul, add.  Here the rank-r (<=256) reduction runs as one MFMA
// kernel that accumulates STRAIGHT INTO the main GEMM's output, with the
// dropout mask generated once (philox4x32-10, packed bits) and re-applied
// in backward — removing three [M,N]-sized memory round trips per wrapped
// Linear per direction:
//
//   fwd:  y[M,N]  += t[M,r] @ Bs[N,r]^T          (lora_add, TRANSQ=false)
//   bwd:  dx[M,K] += mask/(1-p) * (u[M,r] @ A[r,K])   (TRANSQ=true, MASK)
//
// Tile: 128x128 out per 256-thread block (4 waves, 64x64 per wave),
// mfma_f32_16x16x32_bf16, whole r staged in LDS once (no K loop over
// tiles: r <= 256).  Operand tiles are staged row-major with a 16-byte row
// pad (the attention kernels' proven layout) and read as contiguous-k
// bf16x8 fragments.

#include <climits>

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// Default: 8-element row padding (staging writes conflict-free, fragment
// reads 2-way per the bank model).  RELORA_AMD_ROT_V2: zero padding + a
// per-row XOR swizzle on row-major tiles — conflict-free on every modeled
// pattern for r % 64 == 0 (the flagship r=128 included); see
// tools/lds_bank_model.py and tests/test_lds_bank_model.py.
#ifdef RELORA_AMD_ROT_V2
#define LPAD 0
#else
#define LPAD 8  // bf16 elements of LDS row padding (one 16B slot)
#endif

DEV_INLINE int rm_swz(int row, int ldst) {
#ifdef RELORA_AMD_ROT_V2
  return ((ldst & 127) == 0 ? (row & 15) : (row & 7)) << 3;
#else
  (void)row; (void)ldst;
  return 0;
#endif
}
// swizzled element index into a row-major [R][ldst] LDS tile — every
// producer and consumer must address through this
DEV_INLINE int rm_idx(int row, int col, int ldst) {
  return (row * ldst + col) ^ rm_swz(row, ldst);
}

// Rotated layout for transposed LDS tiles with 64-element rows: element
// (row, c) of an [R][64] image lives at row*64 + rot8(row, c), with the
// rotation verified by the in-tree bank model (tools/lds_bank_model.py):
// writes and reads cap at 2-way with zero padding (the naive layout was
// 8-way — 44% of skinny_grad wave cycles).  RELORA_AMD_ROT_V2 switches to
// the Q_V2 table (conflict-free reads, writes stay at the 2-way floor);
// numerics-neutral — writer and reader share the one bijection.
#ifdef RELORA_AMD_ROT_V2
__device__ constexpr unsigned char Q_V2_L[16][8] = {
    {4, 2, 0, 3, 6, 1, 7, 5}, {6, 0, 3, 4, 1, 5, 2, 7},
    {0, 6, 5, 1, 7, 3, 4, 2}, {0, 6, 1, 7, 5, 2, 3, 4},
    {1, 5, 2, 7, 6, 4, 0, 3}, {2, 5, 3, 0, 1, 4, 6, 7},
    {4, 6, 5, 3, 0, 1, 7, 2}, {1, 4, 2, 6, 7, 3, 5, 0},
    {3, 1, 7, 4, 5, 2, 6, 0}, {7, 3, 0, 5, 6, 2, 1, 4},
    {5, 7, 4, 6, 2, 0, 3, 1}, {3, 1, 6, 4, 0, 7, 2, 5},
    {2, 0, 1, 6, 3, 7, 5, 4}, {7, 4, 2, 5, 6, 3, 1, 0},
    {3, 7, 2, 0, 5, 4, 6, 1}, {2, 5, 7, 1, 0, 4, 6, 3}};
DEV_INLINE int rot8(int row, int c64) {
  return (((Q_V2_L[row & 15][c64 >> 3] + 2 * (row >> 4)) & 7) << 3) + (c64 & 7);
}
#else
DEV_INLINE int rot8(int row, int c64) {
  return ((((c64 >> 3) + (row >> 3) + (row & 7)) & 7) << 3) + (c64 & 7);
}
#endif
DEV_INLINE int tr64(int row, int c) { return row * 64 + rot8(row, c); }

// In-row offset for a TRANSQ (transposed) tile element at column k of a row
// with r k-elements.  Default: 64-element blocks with the 8-deep rot8
// rotation.  Under RELORA_AMD_ROT_V2 with r a multiple of 128 (256-byte
// rows), an 8-deep rotation is pigeonhole-bound to 2-way fragment reads,
// so use the closed-form 16-deep whole-row permutation instead (verified
// conflict-free reads + floor writes by the in-tree bank model).  The
// writer and reader share this one mapping, so the choice is
// numerics-neutral.
#ifdef RELORA_AMD_ROT_V2
__device__ constexpr unsigned char X16_TRQ[16] = {
    0, 2, 4, 6, 1, 3, 5, 7, 9, 11, 13, 15, 8, 10, 12, 14};
DEV_INLINE int trq_off(int row, int k, int r) {
  if ((r & 127) == 0) {
    const int grp = (k & 127) >> 3;
    const int p = (X16_TRQ[row & 15] + ((grp & 1) << 3) + (grp >> 1) +
                   2 * (row >> 4)) & 15;
    return (k & ~127) + p * 8 + (k & 7);
  }
  return (k & ~63) + rot8(row, k & 63);
}
#else
DEV_INLINE int trq_off(int row, int k, int r) {
  (void)r;
  return (k & ~63) + rot8(row, k & 63);
}
#endif


// ---------------------------------------------------------------------------
// philox4x32-10 — counter-based RNG for the dropout mask (regenerable, but we
// persist packed bits: exact replay in backward with zero recompute).
// ---------------------------------------------------------------------------

DEV_INLINE void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                             uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0;
  uint32_t h1 = __umulhi(M1, c2), l1 = M1 * c2;
  uint32_t n0 = h1 ^ c1 ^ k0, n1 = l1, n2 = h0 ^ c3 ^ k1, n3 = l0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

DEV_INLINE void philox4(uint64_t seed, uint64_t idx, uint32_t out[4]) {
  uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = 0x9E3779B9u, c3 = 0xBB67AE85u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// xd = keep ? x/(1-p) : 0; mask bit j of byte [m][k8] = keep(k8*8+j).
// One thread per 8 consecutive elements (one mask byte, one bf16x8 store).
template <typename T>
__global__ void dropout_mask_kernel(const T* __restrict__ x, T* __restrict__ xd,
                                    uint8_t* __restrict__ mask, long n8, long n,
                                    uint64_t seed, float p, float inv_keep) {
  const long i8 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i8 >= n8) return;
  uint32_t r[4];
  philox4(seed, (uint64_t)i8, r);
  const uint32_t thr = (uint32_t)(p * 65536.0f);
  const uint32_t u16s[8] = {r[0] & 0xFFFFu, r[0] >> 16, r[1] & 0xFFFFu, r[1] >> 16,
                            r[2] & 0xFFFFu, r[2] >> 16, r[3] & 0xFFFFu, r[3] >> 16};
  if (i8 * 8 + 8 <= n) {
    Vec8<T> v = load8(x + i8 * 8);
    Vec8<T> o;
    uint8_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool keep = u16s[j] >= thr;
      m |= (uint8_t)keep << j;
      o.v[j] = keep ? from_f32<T>(to_f32(v.v[j]) * inv_keep) : from_f32<T>(0.f);
    }
    store8(xd + i8 * 8, o);
    mask[i8] = m;
  } else {  // tail: < 8 elements
    uint8_t m = 0;
    for (int j = 0; j < 8 && i8 * 8 + j < n; ++j) {
      const bool keep = u16s[j] >= thr;
      m |= (uint8_t)keep << j;
      xd[i8 * 8 + j] = keep ? from_f32<T>(to_f32(x[i8 * 8 + j]) * inv_keep)
                            : from_f32<T>(0.f);
    }
    mask[i8] = m;
  }
}

// backward of the packed-mask dropout: dx = dy * mask * inv_keep
template <typename T>
__global__ void mask_apply_kernel(const T* __restrict__ dy, T* __restrict__ dx,
                                  const uint8_t* __restrict__ mask, long n8,
                                  long n, float inv_keep) {
  const long i8 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i8 >= n8) return;
  const uint8_t m = mask[i8];
  if (i8 * 8 + 8 <= n) {
    Vec8<T> v = load8(dy + i8 * 8);
    Vec8<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o.v[j] = ((m >> j) & 1) ? from_f32<T>(to_f32(v.v[j]) * inv_keep)
                              : from_f32<T>(0.f);
    store8(dx + i8 * 8, o);
  } else {
    for (int j = 0; j < 8 && i8 * 8 + j < n; ++j)
      dx[i8 * 8 + j] = ((m >> j) & 1)
                           ? from_f32<T>(to_f32(dy[i8 * 8 + j]) * inv_keep)
                           : from_f32<T>(0.f);
  }
}

// ---------------------------------------------------------------------------
// rank-r accumulate kernel
// out[M,N] (+)= P[M,r] @ Q^T          (TRANSQ=false: Q is [N,r] row-major)
// out[M,N] (+)= maskscale * (P[M,r] @ Q)   (TRANSQ=true: Q is [r,N] row-major)
// ---------------------------------------------------------------------------

template <bool TRANSQ, bool MASK>
__global__ __launch_bounds__(256) void lora_skinny_kernel(
    const __hip_bfloat16* __restrict__ P, const __hip_bfloat16* __restrict__ Q,
    __hip_bfloat16* __restrict__ out, const uint8_t* __restrict__ mask,
    float inv_keep, long M, int N, int r, int ldq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldt = r + LPAD;
  __bf16* p_im = (__bf16*)smem;            // [128][ldt]
  // TRANSQ rows hold whole 64-element rotation blocks (trq_off permutes
  // inside them), so their stride rounds r up to a multiple of 64
  const int ldq_t = TRANSQ ? ((r + 63) & ~63) + LPAD : ldt;
  __bf16* q_im = p_im + 128 * ldt;         // [128][ldt], TRANSQ: [128][ldq_t]

  const long m0 = (long)blockIdx.y * 128;
  const int n0 = blockIdx.x * 128;

  // stage P rows [128][r]
  for (int t = threadIdx.x; t < 128 * (r / 8); t += blockDim.x) {
    const int row = t / (r / 8);
    const int c = (t % (r / 8)) * 8;
    bf16x8 v;
    if (m0 + row < M) {
      v = *reinterpret_cast<const bf16x8*>(P + (m0 + row) * (long)r + c);
    } else {
      v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    *reinterpret_cast<bf16x8*>(p_im + rm_idx(row, c, ldt)) = v;
  }
  // stage Q tile as q_im[n][k]
  if (!TRANSQ) {
    for (int t = threadIdx.x; t < 128 * (r / 8); t += blockDim.x) {
      const int n = t / (r / 8);
      const int c = (t % (r / 8)) * 8;
      bf16x8 v;
      if (n0 + n < N) {
        v = *reinterpret_cast<const bf16x8*>(Q + (n0 + n) * (long)ldq + c);
      } else {
        v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
      *reinterpret_cast<bf16x8*>(q_im + rm_idx(n, c, ldt)) = v;
    }
  } else {
    // Q is [r][N]: q_im[n][k] = Q[k][n0+n].  bf16x8 loads along n (contiguous
    // in global), 8 rotated scalar LDS writes each (conflict-free, see tr64)
    for (int t = threadIdx.x; t < r * 16; t += blockDim.x) {
      const int k = t / 16;
      const int nb = (t % 16) * 8;
      bf16x8 v;
      if (n0 + nb + 8 <= N) {
        v = *reinterpret_cast<const bf16x8*>(Q + (long)k * ldq + n0 + nb);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (n0 + nb + j < N) ? (__bf16)Q[(long)k * ldq + n0 + nb + j] : (__bf16)0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        q_im[(nb + j) * ldq_t + trq_off(nb + j, k, r)] = v[j];
    }
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 64;  // wave row offset in tile
  const int wc = (wave & 1) * 64;   // wave col offset
  const int fr = lane & 15;         // fragment row/col
  const int kg = (lane >> 4) * 8;   // k-group offset

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kk = 0; kk < r; kk += 32) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const bf16x8 a =
          *reinterpret_cast<const bf16x8*>(p_im + rm_idx(wr + mi * 16 + fr, kk + kg, ldt));
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int qrow = wc + ni * 16 + fr;
        const int koff = kk + kg;
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(
            TRANSQ ? q_im + qrow * ldq_t + trq_off(qrow, koff, r)
                   : q_im + rm_idx(qrow, koff, ldt));
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[mi][ni], 0, 0, 0);
      }
    }
  }

  // epilogue in two phases: dump the C-layout accumulators into an LDS
  // [128][136] tile (cheap strided b16 writes), then vectorized bf16x8
  // global read-modify-writes — the per-element C-layout RMW was 64 scalar
  // global round trips per thread
  __syncthreads();  // done with p_im/q_im; reuse the LDS as the out tile
  __bf16* o_im = (__bf16*)smem;  // [128][OLD]
  constexpr int OLD = 128 + LPAD;
  const int crow = (lane >> 4) * 4;  // C-frag rows crow..crow+3, col = fr
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o_im[rm_idx(wr + mi * 16 + crow + j, wc + ni * 16 + fr, OLD)] =
            (__bf16)acc[mi][ni][j];
  __syncthreads();

  for (int t = threadIdx.x; t < 128 * 16; t += blockDim.x) {
    const int row = t / 16;
    const int c8 = (t % 16) * 8;
    const long m = m0 + row;
    const int n = n0 + c8;
    if (m >= M || n >= N) continue;
    const __bf16* src_v = o_im + rm_idx(row, c8, OLD);
    const long flat = m * (long)N + n;  // mask bits are FLAT-packed over [M*N]
    __hip_bfloat16* o = out + flat;
    if (n + 8 <= N && (flat & 7) == 0) {
      Vec8<__hip_bfloat16> ov = load8(o);
      uint8_t mb = 0xFF;
      if (MASK) mb = mask[flat >> 3];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = (float)src_v[j];
        if (MASK) v = (mb >> j) & 1 ? v * inv_keep : 0.f;
        ov.v[j] = from_f32<__hip_bfloat16>(to_f32(ov.v[j]) + v);
      }
      store8(o, ov);
    } else {  // unaligned rows (odd N) or the row tail
      for (int j = 0; j < 8 && n + j < N; ++j) {
        float v = (float)src_v[j];
        if (MASK) {
          const uint8_t mb = mask[(flat + j) >> 3];
          v = (mb >> ((flat + j) & 7)) & 1 ? v * inv_keep : 0.f;
        }
        o[j] = from_f32<__hip_bfloat16>(to_f32(o[j]) + v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

std::vector<torch::Tensor> dropout_mask_fwd(torch::Tensor x, double p, int64_t seed) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "dropout_mask_fwd: bf16 only");
  auto xd = torch::empty_like(x);
  const long n = x.numel();
  const long n8 = (n + 7) / 8;  // FLAT packing: mask bit j of byte b = elem 8b+j
  auto mask = torch::empty({n8}, x.options().dtype(torch::kUInt8));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const float inv_keep = 1.f / (1.f - (float)p);
  hipLaunchKernelGGL(dropout_mask_kernel<__hip_bfloat16>,
                     dim3((n8 + 255) / 256), dim3(256), 0, stream,
                     (const __hip_bfloat16*)x.data_ptr(), (__hip_bfloat16*)xd.data_ptr(),
                     mask.data_ptr<uint8_t>(), n8, n, (uint64_t)seed, (float)p, inv_keep);
  HIP_CHECK_LAST();
  return {xd, mask};
}

// out[M,N] += P[M,r] @ Q[N,r]^T  (forward epilogue; Q = scale*lora_B.weight)
void lora_add_nt_(torch::Tensor out, torch::Tensor P, torch::Tensor Q) {
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && P.is_contiguous() && Q.is_contiguous());
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16, "lora_add: bf16 only");
  const long M = out.size(0);
  const int N = out.size(1);
  const int r = P.size(1);
  TORCH_CHECK(P.size(0) == M && Q.size(0) == N && Q.size(1) == r);
  TORCH_CHECK(r % 32 == 0 && r <= 256, "lora_add: r must be a multiple of 32, <=256");
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = std::max<size_t>(2u * 128 * (r + LPAD), 128u * (128 + LPAD))
                     * sizeof(__bf16);
  dim3 grid((N + 127) / 128, (M + 127) / 128), block(256);
  hipLaunchKernelGGL((lora_skinny_kernel<false, false>), grid, block, lds, stream,
                     (const __hip_bfloat16*)P.data_ptr(), (const __hip_bfloat16*)Q.data_ptr(),
                     (__hip_bfloat16*)out.data_ptr(), nullptr, 1.f, M, N, r, r);
  HIP_CHECK_LAST();
}

// ---------------------------------------------------------------------------
// Group form of the forward epilogue with RoPE: out_g[M,N_g] += P_g[M,r] @
// Q_g[N_g,r]^T for G <= 3 siblings (q/k/v) in ONE launch, and for the siblings
// flagged rotary the rotation is applied to the summed tile before it is
// stored — the separate rope pass over q and k (read y, write a new tensor)
// disappears.
//
// Same 128x128 tile, staging, MFMA loop and bf16 [128][136] LDS out tile as
// lora_skinny_kernel<false,false>.  The siblings share nothing (P_g, Q_g and
// out_g all differ), so the grid is flat over the concatenated column tiles of
// all siblings: blockIdx.x -> (sibling, column tile); a loop over siblings
// inside the block would reuse no operand and only cut the block count by G.
//
// Epilogue: a thread owns 4 (row, 8-column group) pairs: group c in the first
// half of a head and its partner c + hd/2; with hd 64 or 128 and N_g % 128 == 0
// both lie in this tile.  The two bf16x8 of out are loaded before the staging
// and MFMA work (8 loads in flight under it), the update is added and rounded
// to bf16 exactly as lora_add_nt_ does, and the rotation works on those bf16
// values with rope_rotate (common.h): the stored bits equal lora_add_nt_
// followed by rope_fwd.  Non-rotary siblings (v) skip the rotation only.
// The position of row m is m % S (out_g is [B*S, N_g]); cos/sin are the fp32
// [S_cache, hd] tables of rope.hip (R == hd).
// ---------------------------------------------------------------------------

struct LoraRopeGroupArgs {
  const __hip_bfloat16* P[3];
  const __hip_bfloat16* Q[3];
  __hip_bfloat16* out[3];
  int N[3];
  int tile0[3];   // first flat column tile of sibling g (INT_MAX when g >= G)
  int rotary[3];
};

__global__ __launch_bounds__(256, 2) void lora_skinny_rope_group_kernel(
    LoraRopeGroupArgs a, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    long M, int r, int S, int hd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldt = r + LPAD;
  __bf16* p_im = (__bf16*)smem;       // [128][ldt]
  __bf16* q_im = p_im + 128 * ldt;    // [128][ldt]

  // sibling and column tile of this block (selects, not indexing: the
  // argument struct stays in scalar registers)
  const int bx = blockIdx.x;
  const int g = bx >= a.tile0[2] ? 2 : (bx >= a.tile0[1] ? 1 : 0);
  const __hip_bfloat16* P = g == 0 ? a.P[0] : (g == 1 ? a.P[1] : a.P[2]);
  const __hip_bfloat16* Q = g == 0 ? a.Q[0] : (g == 1 ? a.Q[1] : a.Q[2]);
  __hip_bfloat16* out = g == 0 ? a.out[0] : (g == 1 ? a.out[1] : a.out[2]);
  const int N = g == 0 ? a.N[0] : (g == 1 ? a.N[1] : a.N[2]);
  const int tile0 = g == 0 ? a.tile0[0] : (g == 1 ? a.tile0[1] : a.tile0[2]);
  const bool rotary = (g == 0 ? a.rotary[0] : (g == 1 ? a.rotary[1] : a.rotary[2])) != 0;

  const long m0 = (long)blockIdx.y * 128;
  const int n0 = (bx - tile0) * 128;
  const int mrem = (int)min(M - m0, 128L);  // valid rows of the tile

  // this thread's pairs: rows prow + 32 i, columns c .. c+7 and c+half .. +7
  const int prow = threadIdx.x >> 3;
  const int u = threadIdx.x & 7;
  const int half = hd >> 1;
  const int hg = hd >> 4;              // 8-column groups per half head: 4 or 8
  const int ci = (u & (hg - 1)) * 8;   // column inside the half head
  const int c = (u / hg) * hd + ci;
  __hip_bfloat16* obase = out + m0 * (long)N + n0 + c;
  Vec8<__hip_bfloat16> y1[4], y2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = prow + i * 32;
    if (row < mrem) {
      y1[i] = load8(obase + (long)row * N);
      y2[i] = load8(obase + (long)row * N + half);
    }
  }

  // stage P rows [128][r] and the Q tile as q_im[n][k]
  for (int t = threadIdx.x; t < 128 * (r / 8); t += blockDim.x) {
    const int row = t / (r / 8);
    const int k8 = (t % (r / 8)) * 8;
    bf16x8 v;
    if (row < mrem) {
      v = *reinterpret_cast<const bf16x8*>(P + (m0 + row) * (long)r + k8);
    } else {
      v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    *reinterpret_cast<bf16x8*>(p_im + rm_idx(row, k8, ldt)) = v;
  }
  for (int t = threadIdx.x; t < 128 * (r / 8); t += blockDim.x) {
    const int n = t / (r / 8);
    const int k8 = (t % (r / 8)) * 8;
    // N % 128 == 0: every row of the tile exists
    *reinterpret_cast<bf16x8*>(q_im + rm_idx(n, k8, ldt)) =
        *reinterpret_cast<const bf16x8*>(Q + (n0 + n) * (long)r + k8);
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 64;  // wave row offset in tile
  const int wc = (wave & 1) * 64;   // wave col offset
  const int fr = lane & 15;         // fragment row/col
  const int kg = (lane >> 4) * 8;   // k-group offset

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kk = 0; kk < r; kk += 32) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const bf16x8 av =
          *reinterpret_cast<const bf16x8*>(p_im + rm_idx(wr + mi * 16 + fr, kk + kg, ldt));
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(
            q_im + rm_idx(wc + ni * 16 + fr, kk + kg, ldt));
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[mi][ni], 0, 0, 0);
      }
    }
  }

  __syncthreads();  // done with p_im/q_im; reuse the LDS as the out tile
  __bf16* o_im = (__bf16*)smem;  // [128][OLD]
  constexpr int OLD = 128 + LPAD;
  const int crow = (lane >> 4) * 4;  // C-frag rows crow..crow+3, col = fr
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o_im[rm_idx(wr + mi * 16 + crow + j, wc + ni * 16 + fr, OLD)] =
            (__bf16)acc[mi][ni][j];
  __syncthreads();

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = prow + i * 32;
    if (row >= mrem) continue;
    const bf16x8 u1 = *reinterpret_cast<const bf16x8*>(o_im + rm_idx(row, c, OLD));
    const bf16x8 u2 = *reinterpret_cast<const bf16x8*>(o_im + rm_idx(row, c + half, OLD));
    Vec8<__hip_bfloat16> o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o1.v[j] = from_f32<__hip_bfloat16>(to_f32(y1[i].v[j]) + (float)u1[j]);
      o2.v[j] = from_f32<__hip_bfloat16>(to_f32(y2[i].v[j]) + (float)u2[j]);
    }
    if (rotary) {
      const long s = (m0 + row) % S;
      const Vec8<float> cs = load8(cos_t + s * hd + ci);
      const Vec8<float> sn = load8(sin_t + s * hd + ci);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float r1, r2;
        rope_rotate<false>(to_f32(o1.v[j]), to_f32(o2.v[j]), cs.v[j], sn.v[j], r1, r2);
        o1.v[j] = from_f32<__hip_bfloat16>(r1);
        o2.v[j] = from_f32<__hip_bfloat16>(r2);
      }
    }
    store8(obase + (long)row * N, o1);
    store8(obase + (long)row * N + half, o2);
  }
}

// outs[g][M,N_g] += Ps[g][M,r] @ Qs[g][N_g,r]^T for G = 1..3 siblings in one
// launch; siblings with rotary[g] != 0 are RoPE-rotated in place (heads of hd
// columns, position of row m = m % S, cos/sin fp32 [S_cache, hd]).
void lora_add_nt_rope_group_(std::vector<torch::Tensor> outs, std::vector<torch::Tensor> Ps,
                             std::vector<torch::Tensor> Qs, std::vector<int64_t> rotary,
                             torch::Tensor cos_t, torch::Tensor sin_t, int64_t S,
                             int64_t hd) {
  const int G = (int)outs.size();
  TORCH_CHECK(G >= 1 && G <= 3 && (int)Ps.size() == G && (int)Qs.size() == G &&
              (int)rotary.size() == G,
              "lora_add_nt_rope_group_: 1..3 siblings, one P, Q and flag per out");
  TORCH_CHECK(hd == 64 || hd == 128, "lora_add_nt_rope_group_: head_dim must be 64 or 128");
  TORCH_CHECK(cos_t.is_cuda() && sin_t.is_cuda() && cos_t.dim() == 2 &&
              cos_t.scalar_type() == torch::kFloat32 &&
              sin_t.scalar_type() == torch::kFloat32 && cos_t.is_contiguous() &&
              sin_t.is_contiguous() && sin_t.sizes() == cos_t.sizes() &&
              ((uintptr_t)cos_t.data_ptr() & 15) == 0 && ((uintptr_t)sin_t.data_ptr() & 15) == 0,
              "lora_add_nt_rope_group_: cos/sin must be contiguous fp32 [S_cache, hd]");
  TORCH_CHECK(cos_t.size(1) == hd, "lora_add_nt_rope_group_: full rotary only (R == head_dim)");
  TORCH_CHECK(S >= 1 && cos_t.size(0) >= S, "rope cache shorter than sequence");
  TORCH_CHECK(Ps[0].dim() == 2, "lora_add_nt_rope_group_: P_g must be [M,r]");
  const long M = Ps[0].size(0);
  const int r = Ps[0].size(1);
  TORCH_CHECK(r % 32 == 0 && r <= 128,
              "lora_add_nt_rope_group_: r must be a multiple of 32, <= 128");
  LoraRopeGroupArgs a = {};
  int tiles = 0;
  for (int g = 0; g < 3; ++g) a.tile0[g] = INT_MAX;
  for (int g = 0; g < G; ++g) {
    const auto& out = outs[g];
    const auto& P = Ps[g];
    const auto& Q = Qs[g];
    TORCH_CHECK(out.is_cuda() && P.is_cuda() && Q.is_cuda() && out.is_contiguous() &&
                P.is_contiguous() && Q.is_contiguous() &&
                out.scalar_type() == torch::kBFloat16 &&
                P.scalar_type() == torch::kBFloat16 && Q.scalar_type() == torch::kBFloat16,
                "lora_add_nt_rope_group_: out_g, P_g, Q_g must be contiguous bf16");
    TORCH_CHECK(out.dim() == 2 && P.dim() == 2 && Q.dim() == 2 && out.size(0) == M &&
                P.size(0) == M && P.size(1) == r && Q.size(1) == r &&
                Q.size(0) == out.size(1),
                "lora_add_nt_rope_group_: shape mismatch");
    const long N = out.size(1);
    TORCH_CHECK(N % 128 == 0 && N % hd == 0 && N < (1L << 24),
                "lora_add_nt_rope_group_: N_g must be a multiple of 128");
    TORCH_CHECK(((uintptr_t)out.data_ptr() & 15) == 0 && ((uintptr_t)P.data_ptr() & 15) == 0 &&
                ((uintptr_t)Q.data_ptr() & 15) == 0,
                "lora_add_nt_rope_group_: 16-byte aligned tensors only");
    a.out[g] = (__hip_bfloat16*)out.data_ptr();
    a.P[g] = (const __hip_bfloat16*)P.data_ptr();
    a.Q[g] = (const __hip_bfloat16*)Q.data_ptr();
    a.N[g] = (int)N;
    a.rotary[g] = rotary[g] != 0;
    a.tile0[g] = tiles;
    tiles += (int)(N / 128);
  }
  if (M == 0) return;
  TORCH_CHECK((M + 127) / 128 <= 65535, "lora_add_nt_rope_group_: too many rows");
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = std::max<size_t>(2u * 128 * (r + LPAD), 128u * (128 + LPAD))
                     * sizeof(__bf16);
  dim3 grid(tiles, (M + 127) / 128), block(256);
  hipLaunchKernelGGL(lora_skinny_rope_group_kernel, grid, block, lds, stream, a,
                     cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), M, r, (int)S, (int)hd);
  HIP_CHECK_LAST();
}

// out[M,K] += maskscale * (P[M,r] @ Q[r,K])  (backward dx epilogue; Q = lora_A.weight)
void lora_add_nn_(torch::Tensor out, torch::Tensor P, torch::Tensor Q,
                  torch::Tensor mask, double inv_keep) {
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && P.is_contiguous() && Q.is_contiguous());
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16, "lora_add: bf16 only");
  const long M = out.size(0);
  const int N = out.size(1);
  const int r = P.size(1);
  TORCH_CHECK(P.size(0) == M && Q.size(0) == r && Q.size(1) == N);
  TORCH_CHECK(r % 32 == 0 && r <= 256, "lora_add: r must be a multiple of 32, <=256");
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = std::max<size_t>(128u * (r + LPAD) + 128u * (((r + 63) & ~63) + LPAD),
                                      128u * (128 + LPAD)) * sizeof(__bf16);
  dim3 grid((N + 127) / 128, (M + 127) / 128), block(256);
  const bool has_mask = mask.defined() && mask.numel() > 0;
  if (has_mask) {
    TORCH_CHECK(mask.numel() == (M * (long)N + 7) / 8, "mask size mismatch");
    hipLaunchKernelGGL((lora_skinny_kernel<true, true>), grid, block, lds, stream,
                       (const __hip_bfloat16*)P.data_ptr(),
                       (const __hip_bfloat16*)Q.data_ptr(),
                       (__hip_bfloat16*)out.data_ptr(), mask.data_ptr<uint8_t>(),
                       (float)inv_keep, M, N, r, N);
  } else {
    hipLaunchKernelGGL((lora_skinny_kernel<true, false>), grid, block, lds, stream,
                       (const __hip_bfloat16*)P.data_ptr(),
                       (const __hip_bfloat16*)Q.data_ptr(),
                       (__hip_bfloat16*)out.data_ptr(), nullptr, 1.f, M, N, r, N);
  }
  HIP_CHECK_LAST();
}

// ---------------------------------------------------------------------------
// Group form of the dx epilogue: out[M,N] += sum_g maskscale_g * (P_g @ Q_g)
// for G <= 3 siblings that accumulate into the same out (q/k/v, gate/up), as
// ONE read-modify-write of out instead of G.
//
// Same 128x128 tile, 4 waves and staging as lora_skinny_kernel<true, MASK>.
// Per sibling: stage P_g and the rotated Q_g^T tile, run the MFMAs, dump the
// C layout through LDS (fp32 here, so a contribution is not rounded before it
// is summed) and add the mask-selected, inv_keep-scaled values into a
// per-thread fp32 running sum laid out like the final bf16x8 pieces (8 pieces
// of 8 per thread).  The out pieces do not depend on any of that, so their
// loads are issued first, in flight under the first sibling's staging and
// MFMA work, and start the running sum; the old out and the G contributions
// are summed in fp32 and rounded once.
// ---------------------------------------------------------------------------

struct LoraAddGroupArgs {
  const __hip_bfloat16* P[3];
  const __hip_bfloat16* Q[3];
  const uint8_t* mask[3];
};

template <bool MASK>
__global__ __launch_bounds__(256, 2) void lora_skinny_group_kernel(
    LoraAddGroupArgs a, int G, __hip_bfloat16* __restrict__ out, float inv_keep,
    long M, int N, int r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ldt = r + LPAD;
  // whole 64-element rotation blocks per transposed row, as lora_skinny_kernel
  const int ldq_t = ((r + 63) & ~63) + LPAD;
  __bf16* p_im = (__bf16*)smem;         // [128][ldt]
  __bf16* q_im = p_im + 128 * ldt;      // [128][ldq_t]
  constexpr int OLDF = 128 + 4;         // fp32 out-tile stride (16 B pad)
  float* o_im = (float*)smem;           // [128][OLDF], aliases p_im/q_im

  const long m0 = (long)blockIdx.y * 128;
  const int n0 = blockIdx.x * 128;

  // this thread's 8 out pieces: rows prow + 16 i, columns n .. n + 7, at
  // 32-bit offsets from the tile's first element (flat index base_flat; mask
  // bits are FLAT-packed over [M*N], so bit base_lo of byte base_flat >> 3)
  const int prow = threadIdx.x >> 4;
  const int c8 = (threadIdx.x & 15) * 8;
  const int n = n0 + c8;
  const long base_flat = m0 * (long)N + n0;
  const unsigned base_lo = (unsigned)(base_flat & 7);
  __hip_bfloat16* obase = out + base_flat;
  const int mrem = (int)min(M - m0, 128L);  // valid rows of the tile
  auto piece_off = [&](int i) { return base_lo + (unsigned)(prow + i * 16) * N + c8; };
  auto piece_ok = [&](int i) { return prow + i * 16 < mrem && n < N; };
  auto piece_vec = [&](int i) {
    return prow + i * 16 < mrem && n + 8 <= N && (piece_off(i) & 7) == 0;
  };
  // fp32 running sum, started from the old out where the piece is one
  // aligned bf16x8 (pieces of the unaligned path start at 0 and add the old
  // values in the final scalar read-modify-write)
  float sum[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (piece_vec(i)) {
      const Vec8<__hip_bfloat16> ov = load8(obase + (piece_off(i) - base_lo));
#pragma unroll
      for (int j = 0; j < 8; ++j) sum[i][j] = to_f32(ov.v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) sum[i][j] = 0.f;
    }
  }

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 64;  // wave row offset in tile
  const int wc = (wave & 1) * 64;   // wave col offset
  const int fr = lane & 15;         // fragment row/col
  const int kg = (lane >> 4) * 8;   // k-group offset
  const int crow = (lane >> 4) * 4; // C-frag rows crow..crow+3, col = fr

  for (int g = 0; g < G; ++g) {
    const __hip_bfloat16* P = g == 0 ? a.P[0] : (g == 1 ? a.P[1] : a.P[2]);
    const __hip_bfloat16* Q = g == 0 ? a.Q[0] : (g == 1 ? a.Q[1] : a.Q[2]);
    const uint8_t* mbase =
        (g == 0 ? a.mask[0] : (g == 1 ? a.mask[1] : a.mask[2])) + (base_flat >> 3);
    if (g) __syncthreads();  // the previous sibling's o_im reads are done

    // stage P rows [128][r]
    for (int t = threadIdx.x; t < 128 * (r / 8); t += blockDim.x) {
      const int row = t / (r / 8);
      const int c = (t % (r / 8)) * 8;
      bf16x8 v;
      if (m0 + row < M) {
        v = *reinterpret_cast<const bf16x8*>(P + (m0 + row) * (long)r + c);
      } else {
        v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
      *reinterpret_cast<bf16x8*>(p_im + rm_idx(row, c, ldt)) = v;
    }
    // Q is [r][N]: q_im[n][k] = Q[k][n0+n], rotated (see lora_skinny_kernel)
    for (int t = threadIdx.x; t < r * 16; t += blockDim.x) {
      const int k = t / 16;
      const int nb = (t % 16) * 8;
      bf16x8 v;
      if (n0 + nb + 8 <= N) {
        v = *reinterpret_cast<const bf16x8*>(Q + (long)k * N + n0 + nb);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = (n0 + nb + j < N) ? (__bf16)Q[(long)k * N + n0 + nb + j] : (__bf16)0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        q_im[(nb + j) * ldq_t + trq_off(nb + j, k, r)] = v[j];
    }
    // mask bytes of the aligned pieces; loaded before the MFMA loop, used
    // after it
    uint32_t mb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      mb[i] = 0xFF;
      if (MASK && piece_vec(i)) mb[i] = mbase[piece_off(i) >> 3];
    }
    __syncthreads();

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < r; kk += 32) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const bf16x8 av =
            *reinterpret_cast<const bf16x8*>(p_im + rm_idx(wr + mi * 16 + fr, kk + kg, ldt));
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int qrow = wc + ni * 16 + fr;
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(
              q_im + qrow * ldq_t + trq_off(qrow, kk + kg, r));
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[mi][ni], 0, 0, 0);
        }
      }
    }

    __syncthreads();  // done with p_im/q_im; reuse the LDS as the out tile
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o_im[(wr + mi * 16 + crow + j) * OLDF + wc + ni * 16 + fr] = acc[mi][ni][j];
    __syncthreads();

#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float* src = o_im + (prow + i * 16) * OLDF + c8;
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(src);
      const f32x4 s1 = *reinterpret_cast<const f32x4*>(src + 4);
      if (MASK && !piece_vec(i) && piece_ok(i)) {
        // unaligned rows (odd N) or the row tail: gather the 8 bits
        const unsigned off = piece_off(i);
        mb[i] = 0;
        for (int j = 0; j < 8 && n + j < N; ++j)
          mb[i] |= ((uint32_t)(mbase[(off + j) >> 3] >> ((off + j) & 7)) & 1u) << j;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = j < 4 ? s0[j] : s1[j - 4];
        if (MASK) sum[i][j] += (mb[i] >> j) & 1 ? v * inv_keep : 0.f;
        else sum[i][j] += v;
      }
    }
  }

  // one read-modify-write of out
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (!piece_ok(i)) continue;
    __hip_bfloat16* o = obase + (piece_off(i) - base_lo);
    if (piece_vec(i)) {
      Vec8<__hip_bfloat16> ov;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov.v[j] = from_f32<__hip_bfloat16>(sum[i][j]);
      store8(o, ov);
    } else {  // unaligned rows (odd N) or the row tail
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (n + j < N) o[j] = from_f32<__hip_bfloat16>(to_f32(o[j]) + sum[i][j]);
    }
  }
}

// out[M,K] += sum_g maskscale * (Ps[g][M,r] @ Qs[g][r,K]), G = 1..3 siblings
// sharing one r; masks empty -> no dropout.  One rounding of out to bf16.
void lora_add_nn_group_(torch::Tensor out, std::vector<torch::Tensor> Ps,
                        std::vector<torch::Tensor> Qs, std::vector<torch::Tensor> masks,
                        double inv_keep) {
  const int G = (int)Ps.size();
  TORCH_CHECK(G >= 1 && G <= 3 && (int)Qs.size() == G,
              "lora_add_nn_group_: 1..3 siblings, one Q per P");
  TORCH_CHECK(masks.empty() || (int)masks.size() == G,
              "lora_add_nn_group_: no masks or one per sibling");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 2,
              "lora_add_nn_group_: out must be a contiguous [M,K] tensor");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16, "lora_add: bf16 only");
  const long M = out.size(0);
  const int N = out.size(1);
  TORCH_CHECK(Ps[0].dim() == 2, "lora_add_nn_group_: P_g must be [M,r]");
  const int r = Ps[0].size(1);
  TORCH_CHECK(r % 32 == 0 && r <= 256, "lora_add: r must be a multiple of 32, <=256");
  const bool has_mask = !masks.empty();
  LoraAddGroupArgs a = {};
  for (int g = 0; g < G; ++g) {
    const auto& P = Ps[g];
    const auto& Q = Qs[g];
    TORCH_CHECK(P.is_cuda() && Q.is_cuda() && P.is_contiguous() && Q.is_contiguous() &&
                P.scalar_type() == torch::kBFloat16 && Q.scalar_type() == torch::kBFloat16,
                "lora_add_nn_group_: P_g, Q_g must be contiguous bf16");
    TORCH_CHECK(P.dim() == 2 && Q.dim() == 2 && P.size(1) == r && Q.size(0) == r,
                "lora_add_nn_group_: every sibling must have the same r");
    TORCH_CHECK(P.size(0) == M && Q.size(1) == N, "lora_add_nn_group_: shape mismatch");
    a.P[g] = (const __hip_bfloat16*)P.data_ptr();
    a.Q[g] = (const __hip_bfloat16*)Q.data_ptr();
    if (has_mask) {
      TORCH_CHECK(masks[g].is_cuda() && masks[g].is_contiguous() &&
                  masks[g].scalar_type() == torch::kUInt8 &&
                  masks[g].numel() == (M * (long)N + 7) / 8, "mask size mismatch");
      a.mask[g] = masks[g].data_ptr<uint8_t>();
    }
  }
  if (M == 0 || N == 0) return;
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = std::max<size_t>(
      (128u * (r + LPAD) + 128u * (((r + 63) & ~63) + LPAD)) * sizeof(__bf16),
      128u * (128 + 4) * sizeof(float));
  dim3 grid((N + 127) / 128, (M + 127) / 128), block(256);
  if (has_mask)
    hipLaunchKernelGGL((lora_skinny_group_kernel<true>), grid, block, lds, stream, a, G,
                       (__hip_bfloat16*)out.data_ptr(), (float)inv_keep, M, N, r);
  else
    hipLaunchKernelGGL((lora_skinny_group_kernel<false>), grid, block, lds, stream, a, G,
                       (__hip_bfloat16*)out.data_ptr(), 1.f, M, N, r);
  HIP_CHECK_LAST();
}

// ---------------------------------------------------------------------------
// LoRA weight gradients: out[r, C] = P[M, r]^T @ X[M, C], fp32 partials per
// M-chunk (deterministic tree sum in the caller).  hipBLASLt runs these
// skinny-output reductions as 32-workgroup launches (12% of the chip);
// chunking M restores full occupancy.
//   dA          = skinny_grad(P=u_s,  X=xd) -> [r, K]
//   dB^T        = skinny_grad(P=t_u,  X=dy) -> [r, N]
// ---------------------------------------------------------------------------

// grid: (C/128, MCHUNKS, r/128); block 256 (4 waves); out tile [128][128].
// MASK: X is consumed as dropout(X) = maskbit * X * inv_keep, applied while
// staging (so the forward never has to persist the dropped-out activations).
template <bool MASK>
__global__ __launch_bounds__(256) void skinny_grad_kernel(
    const __hip_bfloat16* __restrict__ P, const __hip_bfloat16* __restrict__ X,
    const uint8_t* __restrict__ xmask, float inv_keep,
    float* __restrict__ part, long M, int C, int r, int rows_per_chunk) {
  const int r0 = blockIdx.z * 128;      // r-tile (rank 256 spans two)
  const int rtile = min(r - r0, 128);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered rotated tiles; staging for m-tile t+1 overlaps the MFMA
  // work of tile t (one barrier per m-tile — same scheme as attention.hip)
  __bf16* pt = (__bf16*)smem;        // [2][128][64] rotated: P^T tiles
  __bf16* xt = pt + 2 * 128 * 64;    // [2][128][64] rotated: X^T tiles

  const int c0 = blockIdx.x * 128;
  const long m_begin = (long)blockIdx.y * rows_per_chunk;
  const long m_end = min(M, m_begin + rows_per_chunk);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int kgrp = lane >> 4;

  // per-wave output rows: wave*32 .. +32 (2 row frags), cols c0..c0+128
  f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto stage = [&](long m0, int buf) {
    __bf16* ptb = pt + buf * 128 * 64;
    __bf16* xtb = xt + buf * 128 * 64;
    // P^T slice: pt[j][mm] = P[m0+mm][r0+j]
    for (int t = threadIdx.x; t < 64 * (rtile / 8); t += blockDim.x) {
      const int mm = t / (rtile / 8);
      const int j8 = (t % (rtile / 8)) * 8;
      bf16x8 v;
      if (m0 + mm < m_end) {
        v = *reinterpret_cast<const bf16x8*>(P + (m0 + mm) * (long)r + r0 + j8);
      } else {
        v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ptb[tr64(j8 + j, mm)] = v[j];
    }
    // X^T: xt[cc][mm] = X[m0+mm][c0+cc]; vec8 over the row direction
    for (int t = threadIdx.x; t < 64 * 16; t += blockDim.x) {
      const int mm = t / 16;
      const int c8 = (t % 16) * 8;
      bf16x8 v;
      const long xoff = (m0 + mm) * (long)C + c0 + c8;
      if (m0 + mm < m_end && c0 + c8 + 8 <= C && (xoff & 7) == 0) {
        v = *reinterpret_cast<const bf16x8*>(X + xoff);
        if (MASK) {
          // flat-packed bits; an aligned vec8 covers bits j..j+7 of bytes
          // (xoff>>3) and possibly (xoff>>3)+1 when xoff&7 != 0 — here
          // (xoff&7)==0 so exactly one byte
          const uint8_t mb = xmask[xoff >> 3];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            v[j] = (mb >> j) & 1 ? (__bf16)((float)v[j] * inv_keep) : (__bf16)0.f;
        }
      } else if (m0 + mm < m_end) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = (c0 + c8 + j < C) ? (float)(__bf16)X[xoff + j] : 0.f;
          if (MASK && c0 + c8 + j < C) {
            const uint8_t mb = xmask[(xoff + j) >> 3];
            f = (mb >> ((xoff + j) & 7)) & 1 ? f * inv_keep : 0.f;
          }
          v[j] = (__bf16)f;
        }
      } else {
        v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) xtb[tr64(c8 + j, mm)] = v[j];
    }
  };

  stage(m_begin, 0);
  __syncthreads();
  for (long m0 = m_begin; m0 < m_end; m0 += 64) {
    const int buf = (int)(((m0 - m_begin) >> 6) & 1);
    if (m0 + 64 < m_end) stage(m0 + 64, buf ^ 1);
    const __bf16* ptb = pt + buf * 128 * 64;
    const __bf16* xtb = xt + buf * 128 * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int jrow = wave * 32 + i * 16 + col;
        const bf16x8 a = (jrow < rtile)
            ? *reinterpret_cast<const bf16x8*>(ptb + tr64(jrow, ks * 32 + kgrp * 8))
            : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(
              xtb + tr64(j * 16 + col, ks * 32 + kgrp * 8));
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // epilogue: fp32 partial plane for this chunk
  float* plane = part + (long)blockIdx.y * r * C;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rbase = wave * 32 + i * 16 + (kgrp << 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j * 16 + col;
      if (c >= C) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rr = rbase + reg;
        if (rr < rtile) plane[(long)(r0 + rr) * C + c] = acc[i][j][reg];
      }
    }
  }
}

// combine the MCHUNK fp32 partial planes: out = scale * sum_chunks(part),
// emitted in the requested dtype, optionally transposed ([C, r] instead of
// [r, C]) — folds the .sum(0).t().contiguous().mul_(scale).to(bf16) chain
// (5 launches per wrapped Linear) into one kernel.
template <typename T, bool TRANSP>
__global__ void skinny_combine_kernel(const float* __restrict__ part,
                                      T* __restrict__ out, int r, int C,
                                      int nchunks, float scale) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)r * C) return;
  float acc = 0.f;
  for (int c = 0; c < nchunks; ++c) acc += part[(long)c * r * C + i];
  acc *= scale;
  if (TRANSP) {
    const int rr = i / C, cc = i % C;
    out[(long)cc * r + rr] = from_f32<T>(acc);
  } else {
    out[i] = from_f32<T>(acc);
  }
}

// out = scale * (P[M,r]^T @ dropout_mask(X)[M,C]) in `dtype`; [C, r] when
// transpose_out.  `xmask` empty -> X used as-is.
torch::Tensor skinny_grad(torch::Tensor P, torch::Tensor X, torch::Tensor xmask,
                          double inv_keep, double scale,
                          bool transpose_out, torch::ScalarType dtype) {
  TORCH_CHECK(P.is_cuda() && P.is_contiguous() && X.is_contiguous());
  TORCH_CHECK(P.scalar_type() == torch::kBFloat16 && X.scalar_type() == torch::kBFloat16);
  const long M = P.size(0);
  const int r = P.size(1);
  const int C = X.size(1);
  TORCH_CHECK(X.size(0) == M && r % 8 == 0 && r <= 256);
  // chunk M so the grid fills the chip: (C/128)*chunks >= ~512
  int chunks = 1;
  const int ctiles = (C + 127) / 128;
  while (chunks < 32 && ctiles * chunks < 512 && (M + chunks - 1) / chunks > 256)
    chunks <<= 1;
  int rows = (int)((M + chunks - 1) / chunks);
  rows = (rows + 63) / 64 * 64;  // multiple of the m-tile
  chunks = (int)((M + rows - 1) / rows);
  auto part = torch::empty({chunks, r, C}, P.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = (4u * 128 * 64) * sizeof(__bf16);
  dim3 grid(ctiles, chunks, (r + 127) / 128), block(256);
  const bool has_mask = xmask.defined() && xmask.numel() > 0;
  if (has_mask) {
    TORCH_CHECK(xmask.numel() == (M * (long)C + 7) / 8, "skinny_grad mask size");
    hipLaunchKernelGGL((skinny_grad_kernel<true>), grid, block, lds, stream,
                       (const __hip_bfloat16*)P.data_ptr(),
                       (const __hip_bfloat16*)X.data_ptr(),
                       xmask.data_ptr<uint8_t>(), (float)inv_keep,
                       part.data_ptr<float>(), M, C, r, rows);
  } else {
    hipLaunchKernelGGL((skinny_grad_kernel<false>), grid, block, lds, stream,
                       (const __hip_bfloat16*)P.data_ptr(),
                       (const __hip_bfloat16*)X.data_ptr(), nullptr, 1.f,
                       part.data_ptr<float>(), M, C, r, rows);
  }
  HIP_CHECK_LAST();
  auto out = transpose_out
      ? torch::empty({C, r}, P.options().dtype(dtype))
      : torch::empty({r, C}, P.options().dtype(dtype));
  dim3 cgrid(((long)r * C + 255) / 256), cblock(256);
  const float s = (float)scale;
  if (dtype == torch::kBFloat16) {
    if (transpose_out)
      hipLaunchKernelGGL((skinny_combine_kernel<__hip_bfloat16, true>), cgrid, cblock, 0,
                         stream, part.data_ptr<float>(),
                         (__hip_bfloat16*)out.data_ptr(), r, C, chunks, s);
    else
      hipLaunchKernelGGL((skinny_combine_kernel<__hip_bfloat16, false>), cgrid, cblock, 0,
                         stream, part.data_ptr<float>(),
                         (__hip_bfloat16*)out.data_ptr(), r, C, chunks, s);
  } else {
    TORCH_CHECK(dtype == torch::kFloat32, "skinny_grad: bf16 or fp32 output");
    if (transpose_out)
      hipLaunchKernelGGL((skinny_combine_kernel<float, true>), cgrid, cblock, 0, stream,
                         part.data_ptr<float>(), out.data_ptr<float>(), r, C, chunks, s);
    else
      hipLaunchKernelGGL((skinny_combine_kernel<float, false>), cgrid, cblock, 0, stream,
                         part.data_ptr<float>(), out.data_ptr<float>(), r, C, chunks, s);
  }
  HIP_CHECK_LAST();
  return out;
}

// ---------------------------------------------------------------------------
// Group form of the dA gradient: out_g[r, C] = P_g[M, r]^T @ dropout_g(X)[M, C]
// for G <= 3 siblings that share X (q/k/v, gate/up).  Each 64-row x 128-column
// X tile is loaded from global memory ONCE and masked G ways while it is
// staged into G rotated X^T tiles; the P_g^T tiles are staged as in
// skinny_grad_kernel.  Same chunks, m-tiles, k-steps and MFMA as
// skinny_grad_kernel, so every output element sees the same sequence of fp32
// accumulations: the results equal G skinny_grad calls bit for bit.
//
// Block = 512 threads = 8 waves; wave w owns output rows w*16 .. w*16+15 of
// every sibling (8 column fragments each: 32 accumulator registers per
// sibling).  LDS holds ONE buffer of G P^T and G X^T tiles (G * 32 KiB; 96 KiB
// at G = 3, which a double buffer would push past the 160 KiB of a CU).  The
// overlap a second buffer gave comes from registers instead: the global loads
// of m-tile t+1 are issued before the MFMA work of tile t and written to LDS
// after it (two barriers per tile).
//
// grid: (C/128, MCHUNKS, r/128).  part is [chunks][G][r][C] fp32.
// ---------------------------------------------------------------------------

struct SkinnyGroupArgs {
  const __hip_bfloat16* P[3];
  const uint8_t* mask[3];
};

template <int G, bool MASK>
__global__ __launch_bounds__(512) void skinny_grad_group_kernel(
    SkinnyGroupArgs a, const __hip_bfloat16* __restrict__ X, float inv_keep,
    float* __restrict__ part, long M, int C, int r, int rows_per_chunk) {
  constexpr int NX = MASK ? G : 1;      // without masks every sibling reads one X^T
  const int r0 = blockIdx.z * 128;      // r-tile (rank 256 spans two)
  const int rtile = min(r - r0, 128);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* pt = (__bf16*)smem;           // [G][128][64] rotated: P_g^T tiles
  __bf16* xt = pt + G * 128 * 64;       // [NX][128][64] rotated: masked X^T tiles

  const int c0 = blockIdx.x * 128;
  const long m_begin = (long)blockIdx.y * rows_per_chunk;
  const long m_end = min(M, m_begin + rows_per_chunk);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int kgrp = lane >> 4;

  f32x4 acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging pieces of one m-tile, two per thread and tensor:
  //   X: piece t = tid + 512 i -> row t / 16, columns (t % 16) * 8 .. + 7
  //   P_g: piece t -> row t / (rtile / 8), ranks (t % (rtile / 8)) * 8 .. + 7
  const int p8 = rtile / 8;
  bf16x8 xreg[2], preg[G][2];
  uint8_t mreg[NX][2];

  auto gload = [&](long m0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = threadIdx.x + i * 512;
      const int mm = t / 16;
      const int c8 = (t % 16) * 8;
      // 32-bit element offset (the host checks M * C < 2^31); C % 8 == 0, so
      // the 8 mask bits are one byte
      const unsigned xoff = (unsigned)(m0 + mm) * C + c0 + c8;
      if (m0 + mm < m_end && c0 + c8 < C) {
        xreg[i] = *reinterpret_cast<const bf16x8*>(X + xoff);
        if (MASK) {
#pragma unroll
          for (int g = 0; g < NX; ++g) mreg[g][i] = a.mask[g][xoff >> 3];
        }
      } else {
        xreg[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int g = 0; g < NX; ++g) mreg[g][i] = 0;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int t = threadIdx.x + i * 512;
        const int mm = t / p8;
        const int j8 = (t % p8) * 8;
        if (t < 64 * p8 && m0 + mm < m_end) {
          preg[g][i] = *reinterpret_cast<const bf16x8*>(
              a.P[g] + ((unsigned)(m0 + mm) * r + r0 + j8));
        } else {
          preg[g][i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
  };

  auto lstore = [&]() {
    // the LDS addresses below are loop invariants that would be kept in ~32
    // registers across the MFMA work; hiding the thread index from the
    // optimiser has them recomputed per tile (a few VALU ops each) instead
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 512;
        const int mm = t / p8;
        const int j8 = (t % p8) * 8;
        if (t < 64 * p8) {
          __bf16* ptg = pt + g * 128 * 64;
#pragma unroll
          for (int j = 0; j < 8; ++j) ptg[tr64(j8 + j, mm)] = preg[g][i][j];
        }
      }
#pragma unroll
    for (int g = 0; g < NX; ++g)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 512;
        const int mm = t / 16;
        const int c8 = (t % 16) * 8;
        __bf16* xtg = xt + g * 128 * 64;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __bf16 v = xreg[i][j];
          // kept values: the rounding of skinny_grad_kernel, bf16(x * inv_keep)
          if (MASK) v = (mreg[g][i] >> j) & 1 ? (__bf16)((float)v * inv_keep) : (__bf16)0.f;
          xtg[tr64(c8 + j, mm)] = v;
        }
      }
  };

  const int jrow = wave * 16 + col;
  gload(m_begin);
  for (long m0 = m_begin; m0 < m_end; m0 += 64) {
    lstore();
    __syncthreads();
    if (m0 + 64 < m_end) gload(m0 + 64);  // in flight under the MFMA work
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const __bf16* ptg = pt + g * 128 * 64;
        const __bf16* xtg = xt + (MASK ? g : 0) * 128 * 64;
        const bf16x8 av = (jrow < rtile)
            ? *reinterpret_cast<const bf16x8*>(ptg + tr64(jrow, ks * 32 + kgrp * 8))
            : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(
              xtg + tr64(j * 16 + col, ks * 32 + kgrp * 8));
          acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc[g][j], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // the tiles are free for the next lstore
  }

  // epilogue: fp32 partial planes [chunk][g]
  const int rbase = wave * 16 + (kgrp << 2);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float* plane = part + ((long)blockIdx.y * G + g) * r * C;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j * 16 + col;
      if (c >= C) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rr = rbase + reg;
        if (rr < rtile) plane[(long)(r0 + rr) * C + c] = acc[g][j][reg];
      }
    }
  }
}

// out[g][e] = sum_chunks part[chunk][g][e], e over one [r, C] plane; the same
// sequential fp32 sum per element as skinny_combine_kernel
template <typename T>
__global__ void skinny_combine_group_kernel(const float* __restrict__ part,
                                            T* __restrict__ out, long plane, int G,
                                            int nchunks) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane * G) return;
  float acc = 0.f;
  for (int c = 0; c < nchunks; ++c) acc += part[(long)c * G * plane + i];
  out[i] = from_f32<T>(acc);
}

template <int G>
static void launch_skinny_group(bool has_mask, dim3 grid, size_t lds, hipStream_t stream,
                                const SkinnyGroupArgs& a, const __hip_bfloat16* X,
                                float inv_keep, float* part, long M, int C, int r, int rows) {
  if (has_mask)
    hipLaunchKernelGGL((skinny_grad_group_kernel<G, true>), grid, dim3(512), lds, stream, a,
                       X, inv_keep, part, M, C, r, rows);
  else
    hipLaunchKernelGGL((skinny_grad_group_kernel<G, false>), grid, dim3(512), lds, stream, a,
                       X, 1.f, part, M, C, r, rows);
}

// {P_g[M,r]^T @ dropout_mask_g(X)[M,C]} in `dtype`, G = 1..3 siblings sharing X
// and r; the meaning of skinny_grad(P_g, X, mask_g, inv_keep, 1.0, false, dtype)
// per sibling.  masks empty -> X used as-is.  The G results are the planes of
// one [G, r, C] tensor.
std::vector<torch::Tensor> skinny_grad_group(std::vector<torch::Tensor> Ps, torch::Tensor X,
                                             std::vector<torch::Tensor> masks,
                                             double inv_keep, torch::ScalarType dtype) {
  const int G = (int)Ps.size();
  TORCH_CHECK(G >= 1 && G <= 3, "skinny_grad_group: 1..3 siblings");
  TORCH_CHECK(masks.empty() || (int)masks.size() == G,
              "skinny_grad_group: no masks or one per sibling");
  TORCH_CHECK(X.is_cuda() && X.is_contiguous() && X.dim() == 2 &&
              X.scalar_type() == torch::kBFloat16,
              "skinny_grad_group: X must be a contiguous bf16 [M,C] tensor");
  TORCH_CHECK(dtype == torch::kBFloat16 || dtype == torch::kFloat32,
              "skinny_grad: bf16 or fp32 output");
  const long M = X.size(0);
  const int C = X.size(1);
  TORCH_CHECK(Ps[0].dim() == 2, "skinny_grad_group: P_g must be [M,r]");
  const int r = Ps[0].size(1);
  TORCH_CHECK(M >= 1 && C >= 8 && C % 8 == 0,
              "skinny_grad_group: C must be a multiple of 8");
  TORCH_CHECK(M * (long)std::max(C, r) < (1L << 31),
              "skinny_grad_group: M * C must be below 2^31 (32-bit offsets in the kernel)");
  TORCH_CHECK(r % 8 == 0 && r >= 8 && r <= 256, "skinny_grad_group: r % 8 == 0, r <= 256");
  const bool has_mask = !masks.empty();
  SkinnyGroupArgs a = {};
  for (int g = 0; g < G; ++g) {
    const auto& P = Ps[g];
    TORCH_CHECK(P.is_cuda() && P.is_contiguous() && P.scalar_type() == torch::kBFloat16 &&
                P.dim() == 2 && P.size(0) == M, "skinny_grad_group: P_g must be contiguous bf16 [M,r]");
    TORCH_CHECK(P.size(1) == r, "skinny_grad_group: every sibling must have the same r");
    a.P[g] = (const __hip_bfloat16*)P.data_ptr();
    if (has_mask) {
      TORCH_CHECK(masks[g].is_cuda() && masks[g].is_contiguous() &&
                  masks[g].scalar_type() == torch::kUInt8 &&
                  masks[g].numel() == (M * (long)C + 7) / 8, "skinny_grad mask size");
      a.mask[g] = masks[g].data_ptr<uint8_t>();
    }
  }
  // the chunk rule of skinny_grad
  int chunks = 1;
  const int ctiles = (C + 127) / 128;
  while (chunks < 32 && ctiles * chunks < 512 && (M + chunks - 1) / chunks > 256)
    chunks <<= 1;
  int rows = (int)((M + chunks - 1) / chunks);
  rows = (rows + 63) / 64 * 64;  // multiple of the m-tile
  chunks = (int)((M + rows - 1) / rows);
  const long plane = (long)r * C;
  auto part = torch::empty({chunks, G, r, C}, X.options().dtype(torch::kFloat32));
  auto out = torch::empty({G, r, C}, X.options().dtype(dtype));
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = (size_t)(G + (has_mask ? G : 1)) * 128 * 64 * sizeof(__bf16);
  dim3 grid(ctiles, chunks, (r + 127) / 128);
  const __hip_bfloat16* xp = (const __hip_bfloat16*)X.data_ptr();
  switch (G) {
    case 1: launch_skinny_group<1>(has_mask, grid, lds, stream, a, xp, (float)inv_keep,
                                   part.data_ptr<float>(), M, C, r, rows); break;
    case 2: launch_skinny_group<2>(has_mask, grid, lds, stream, a, xp, (float)inv_keep,
                                   part.data_ptr<float>(), M, C, r, rows); break;
    default: launch_skinny_group<3>(has_mask, grid, lds, stream, a, xp, (float)inv_keep,
                                    part.data_ptr<float>(), M, C, r, rows); break;
  }
  HIP_CHECK_LAST();
  dim3 cgrid((plane * G + 255) / 256), cblock(256);
  if (dtype == torch::kBFloat16)
    hipLaunchKernelGGL((skinny_combine_group_kernel<__hip_bfloat16>), cgrid, cblock, 0, stream,
                       part.data_ptr<float>(), (__hip_bfloat16*)out.data_ptr(), plane, G,
                       chunks);
  else
    hipLaunchKernelGGL((skinny_combine_group_kernel<float>), cgrid, cblock, 0, stream,
                       part.data_ptr<float>(), out.data_ptr<float>(), plane, G, chunks);
  HIP_CHECK_LAST();
  std::vector<torch::Tensor> outs;
  for (int g = 0; g < G; ++g) outs.push_back(out.select(0, g));
  return outs;
}

torch::Tensor dropout_mask_bwd(torch::Tensor dy, torch::Tensor mask, double p) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous());
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16);
  auto dx = torch::empty_like(dy);
  const long n = dy.numel();
  const long n8 = (n + 7) / 8;
  TORCH_CHECK(mask.numel() >= n8, "mask too small");
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const float inv_keep = (float)(1.0 / (1.0 - p));
  hipLaunchKernelGGL(mask_apply_kernel<__hip_bfloat16>,
                     dim3((n8 + 255) / 256), dim3(256), 0, stream,
                     (const __hip_bfloat16*)dy.data_ptr(),
                     (__hip_bfloat16*)dx.data_ptr(),
                     mask.data_ptr<uint8_t>(), n8, n, inv_keep);
  HIP_CHECK_LAST();
  return dx;
}

// ---------------------------------------------------------------------------
// lora_down_dropout: t_g[M,r] = dropout_g(x)[M,K] @ A_g[r,K]^T for G <= 3
// sibling projections that share one input x (q/k/v, gate/up).  x is read
// from HBM ONCE for the whole group; no [M,K] dropped copy is ever written.
//
// Block = 256 threads = 4 waves, 64 rows of x, all G*r output columns.
// Wave w owns rows w*16..w*16+15, so in the 16x16x32 MFMA every lane's A
// operand is exactly one aligned run of 8 consecutive k of one row: one
// dropout_mask_kernel unit (one philox4 call, one mask byte).  The lane
// loads that run straight from global into registers, derives each
// sibling's keep bits with the same philox4(seed_g, flat/8) counter /
// 16-bit lanes / threshold as dropout_mask_kernel, writes the mask byte, and
// forms the dropped operand with the same bf16 rounding
// (from_f32(to_f32(x) * inv_keep)) — every philox value is computed by
// exactly one lane, and the masks are bit-identical to dropout_mask_fwd.
//
// The A_g k-slices (the MFMA B operand, shared by the four waves) are
// staged in LDS as [G*r][32] row-major, double buffered, one barrier per
// k-tile; the next tile's global loads are issued before the MFMA work of
// the current one, and x is prefetched several tiles ahead in registers.  Rows are 64 B = one fragment row, so staging writes
// (thread t -> bytes 16t..16t+15) and fragment reads (lane (n,kg) -> byte
// n*64 + kg*16) both cover one contiguous 1 KiB per wave instruction:
// conflict-free without padding or rotation.
//
// RMAX (128 or 256) bounds the static accumulator array; fragments past the
// runtime r are skipped by wave-uniform branches.  DROP=false (p == 0 or
// eval) skips the philox and writes no mask.
// ---------------------------------------------------------------------------

struct LoraDownArgs {
  const __hip_bfloat16* A[3];
  __hip_bfloat16* t[3];
  uint8_t* mask[3];
  uint64_t seed[3];
};

template <int G, int RMAX, bool DROP>
__global__ __launch_bounds__(256) void lora_down_dropout_kernel(
    const __hip_bfloat16* __restrict__ x, LoraDownArgs a, long M, int K, int r,
    float p, float inv_keep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BK = 32;
  constexpr int NF = RMAX / 16;             // column fragments per sibling
  const int ncols = G * r;                  // LDS tile rows in use
  __bf16* bt = (__bf16*)smem;               // [2][ncols][BK]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int fr = lane & 15;
  const int kg = (lane >> 4) * 8;
  const long row = (long)blockIdx.x * 64 + wave * 16 + fr;
  const bool row_ok = row < M;
  const uint32_t thr = (uint32_t)(p * 65536.0f);

  f32x4 acc[G][NF];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging slots: for sibling g (static) and i < RMAX/64, this thread owns
  // tile row n = tid/4 + 64*i of A_g (while n < r) and k = (tid%4)*8
  constexpr int NSL = RMAX / 64;
  bf16x8 gb[G][NSL];
  const int sn = threadIdx.x >> 2;
  const int sk = (threadIdx.x & 3) * 8;
  auto load_b = [&](int k0) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < NSL; ++i) {
        const int n = sn + i * 64;
        gb[g][i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (n < r && k0 + sk + 8 <= K)
          gb[g][i] = *reinterpret_cast<const bf16x8*>(a.A[g] + (long)n * K + k0 + sk);
      }
  };
  auto store_b = [&](int buf) {
    __bf16* dst = bt + (long)buf * ncols * BK;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int i = 0; i < NSL; ++i) {
        const int n = sn + i * 64;
        if (n < r)
          *reinterpret_cast<bf16x8*>(dst + (g * r + n) * BK + sk) = gb[g][i];
      }
  };
  auto load_x = [&](int k0) {
    Vec8<__hip_bfloat16> v;
    if (row_ok && k0 + kg + 8 <= K) {
      v = load8(x + row * (long)K + k0 + kg);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v.v[j] = from_f32<__hip_bfloat16>(0.f);
    }
    return v;
  };

  // x runs XPF k-tiles ahead in a register ring: with one wave per SIMD the
  // HBM latency of a single 64-byte-per-row tile is not covered by one
  // tile's work, XPF tiles in flight are
  constexpr int XPF = 4;
  Vec8<__hip_bfloat16> xq[XPF];
  load_b(0);
#pragma unroll
  for (int s = 0; s < XPF; ++s) xq[s] = load_x(s * BK);
  store_b(0);
  __syncthreads();

  const int ntiles = (K + BK - 1) / BK;
  for (int kt0 = 0; kt0 < ntiles; kt0 += XPF) {
#pragma unroll
    for (int s = 0; s < XPF; ++s) {
      const int kt = kt0 + s;
      if (kt >= ntiles) break;  // block-uniform
      const int k0 = kt * BK;
      const int buf = kt & 1;
      const bool more = kt + 1 < ntiles;
      const Vec8<__hip_bfloat16> xc = xq[s];
      if (more) load_b(k0 + BK);
      xq[s] = load_x(k0 + XPF * BK);  // zeros, no load, past K
      const bool grp_ok = row_ok && k0 + kg + 8 <= K;  // this lane's 8 elements exist
      const __bf16* bsrc = bt + (long)buf * ncols * BK;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        union { Vec8<__hip_bfloat16> h; bf16x8 v; } op;
        if (DROP) {
          const long i8 = (row * (long)K + k0 + kg) >> 3;
          uint32_t rr[4];
          philox4(a.seed[g], (uint64_t)i8, rr);
          const uint32_t u16s[8] = {rr[0] & 0xFFFFu, rr[0] >> 16, rr[1] & 0xFFFFu,
                                    rr[1] >> 16, rr[2] & 0xFFFFu, rr[2] >> 16,
                                    rr[3] & 0xFFFFu, rr[3] >> 16};
          uint8_t m = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const bool keep = u16s[j] >= thr;
            m |= (uint8_t)keep << j;
            op.h.v[j] = keep ? from_f32<__hip_bfloat16>(to_f32(xc.v[j]) * inv_keep)
                             : from_f32<__hip_bfloat16>(0.f);
          }
          if (grp_ok) a.mask[g][i8] = m;
        } else {
          op.h = xc;
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          if (j * 16 < r) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(
                bsrc + (g * r + j * 16 + fr) * BK + kg);
            acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(op.v, b, acc[g][j], 0, 0, 0);
          }
        }
      }
      if (more) store_b(buf ^ 1);
      __syncthreads();
    }
  }

  // epilogue: C fragment rows crow..crow+3 of this wave's 16, column fr
  const long orow0 = (long)blockIdx.x * 64 + wave * 16 + (lane >> 4) * 4;
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      if (j * 16 < r) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (orow0 + q < M)
            a.t[g][(orow0 + q) * (long)r + j * 16 + fr] =
                from_f32<__hip_bfloat16>(acc[g][j][q]);
      }
    }
}

template <int G, int RMAX>
static void launch_lora_down(bool drop, dim3 grid, size_t lds, hipStream_t stream,
                             const __hip_bfloat16* x, const LoraDownArgs& a,
                             long M, int K, int r, float p, float inv_keep) {
  if (drop)
    hipLaunchKernelGGL((lora_down_dropout_kernel<G, RMAX, true>), grid, dim3(256), lds,
                       stream, x, a, M, K, r, p, inv_keep);
  else
    hipLaunchKernelGGL((lora_down_dropout_kernel<G, RMAX, false>), grid, dim3(256), lds,
                       stream, x, a, M, K, r, 0.f, 1.f);
}

// x[M,K], As = G x [r,K], seeds = G philox seeds -> {t_0..t_{G-1}} followed,
// when p > 0, by {mask_0..mask_{G-1}} (FLAT-packed, as dropout_mask_fwd).
// p == 0: no masks, seeds ignored.
std::vector<torch::Tensor> lora_down_dropout(torch::Tensor x, std::vector<torch::Tensor> As,
                                             std::vector<int64_t> seeds, double p) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "lora_down_dropout: bf16 only");
  const int G = (int)As.size();
  TORCH_CHECK(G >= 1 && G <= 3, "lora_down_dropout: 1..3 siblings");
  const bool drop = p > 0.0;
  TORCH_CHECK(p >= 0.0 && p < 1.0, "lora_down_dropout: p in [0,1)");
  TORCH_CHECK(!drop || (int)seeds.size() == G, "lora_down_dropout: one seed per sibling");
  TORCH_CHECK(As[0].dim() == 2, "lora_down_dropout: A_g must be contiguous bf16 [r,K]");
  const long M = x.size(0);
  const int K = x.size(1);
  const int r = As[0].size(0);
  TORCH_CHECK(M >= 1 && K % 8 == 0, "lora_down_dropout: K must be a multiple of 8");
  TORCH_CHECK(r % 32 == 0 && r <= 256, "lora_down_dropout: r must be a multiple of 32, <=256");
  LoraDownArgs a = {};
  std::vector<torch::Tensor> out;
  for (int g = 0; g < G; ++g) {
    TORCH_CHECK(As[g].is_cuda() && As[g].is_contiguous() &&
                As[g].scalar_type() == torch::kBFloat16 && As[g].dim() == 2 &&
                As[g].size(0) == r && As[g].size(1) == K,
                "lora_down_dropout: A_g must be contiguous bf16 [r,K]");
    out.push_back(torch::empty({M, (long)r}, x.options()));
    a.A[g] = (const __hip_bfloat16*)As[g].data_ptr();
    a.t[g] = (__hip_bfloat16*)out[g].data_ptr();
  }
  if (drop) {
    const long n8 = (M * (long)K + 7) / 8;
    for (int g = 0; g < G; ++g) {
      out.push_back(torch::empty({n8}, x.options().dtype(torch::kUInt8)));
      a.mask[g] = out[G + g].data_ptr<uint8_t>();
      a.seed[g] = (uint64_t)seeds[g];
    }
  }
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const size_t lds = 2u * (size_t)G * r * 32 * sizeof(__bf16);
  dim3 grid((unsigned)((M + 63) / 64));
  const __hip_bfloat16* xp = (const __hip_bfloat16*)x.data_ptr();
  const float pf = (float)p;
  const float inv_keep = 1.f / (1.f - pf);
#define LORA_DOWN_CASE(GG)                                                        \
  case GG:                                                                        \
    if (r <= 128) launch_lora_down<GG, 128>(drop, grid, lds, stream, xp, a, M, K, \
                                            r, pf, inv_keep);                     \
    else launch_lora_down<GG, 256>(drop, grid, lds, stream, xp, a, M, K, r, pf,   \
                                   inv_keep);                                     \
    break;
  switch (G) {
    LORA_DOWN_CASE(1)
    LORA_DOWN_CASE(2)
    LORA_DOWN_CASE(3)
  }
#undef LORA_DOWN_CASE
  HIP_CHECK_LAST();
  return out;
}
