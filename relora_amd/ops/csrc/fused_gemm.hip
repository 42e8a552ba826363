#include "hip/hip_runtime.h"
// Fused frozen-GEMM + LoRA rank-r epilogue (K1+K2 — the BASELINE.json
// north-star kernel):  y[M,N] = x[M,K]·W[N,K]^T (+bias) + s·(t[M,r]·Bw[N,r]^T)
// where t = dropout(x)·A^T is produced by the existing skinny LoRA kernel.
//
// Replaces the composed  F.linear (hipBLASLt) + lora_add_nt_  pair on
// aligned shapes: the composed form pays a full [M,N] bf16 read-modify-write
// (the lora_add) on top of the library GEMM; here the rank-r update runs as
// an MFMA epilogue on the resident accumulators (+r/K extra MFMA work, no
// extra [M,N] traffic).
//
// Structure (CDNA4 guide §5 "glds vs register staging", verified tier):
//   256x256 output tile, BK=64, 8 waves (2Mx4N), per-wave 128x64 output,
//   mfma_f32_16x16x32_bf16; both operand tiles staged by
//   global_load_lds_dwordx4 into double-buffered LDS with the st_16x32
//   XOR swizzle applied on the per-lane GLOBAL source address (the LDS
//   image is lane-linear, as glds requires); one vmcnt(0)+barrier per
//   K-tile (the 2-buffer overlap pattern).  All LDS lives in ONE
//   __shared__ array (a second __shared__ object de-pipelines glds).
//
// Constraints (host-checked): M%256==0, N%256==0, K%64==0, r%64==0 (or
// r==0), bf16 contiguous row-major.  Unaligned shapes keep the composed
// library path (llama_1b's intermediate 5461 stays composed; qkvo and the
// whole of llama_250m/llama_7b qualify).

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_g;
typedef __attribute__((ext_vector_type(4))) float f32x4_g;

// ---------------------------------------------------------------------------
// Host checks shared by the five entry points.  The kernels index every
// operand from M, N, K and r alone, so whatever is not checked here is read
// out of bounds on a mismatch.  All of them run before the launch.
// ---------------------------------------------------------------------------

static void check_x(const char* fn, const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda(), fn, ": x must be a GPU tensor");
  TORCH_CHECK(x.dim() == 2, fn, ": x must be 2-D [M, K]");
  TORCH_CHECK(x.is_contiguous(), fn, ": x must be contiguous");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, fn, ": x must be bf16");
  TORCH_CHECK(x.size(0) > 0, fn, ": M must be > 0");
  TORCH_CHECK(x.size(1) > 0, fn, ": K must be > 0");
}

static void check_dense_w(const char* fn, const torch::Tensor& x,
                          const torch::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.device() == x.device(), fn,
              ": w must be on x's device");
  TORCH_CHECK(w.dim() == 2, fn, ": w must be 2-D [N, K]");
  TORCH_CHECK(w.is_contiguous(), fn, ": w must be contiguous");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16, fn, ": w must be bf16");
  TORCH_CHECK(w.size(1) == x.size(1), fn, ": K mismatch between x and w");
  TORCH_CHECK(w.size(0) > 0, fn, ": N must be > 0");
}

// qw holds `qw_numel` codes bytes, amax one fp32 per `block` weights
static void check_quant_w(const char* fn, const torch::Tensor& x,
                          const torch::Tensor& qw, const torch::Tensor& amax,
                          long N, long K, long qw_numel, long block) {
  TORCH_CHECK(N > 0, fn, ": N must be > 0");
  TORCH_CHECK(qw.device() == x.device(), fn, ": qw must be on x's device");
  TORCH_CHECK(qw.is_contiguous(), fn, ": qw must be contiguous");
  TORCH_CHECK(qw.numel() == qw_numel, fn, ": packed weight size mismatch");
  TORCH_CHECK(amax.device() == x.device(), fn, ": absmax must be on x's device");
  TORCH_CHECK(amax.scalar_type() == torch::kFloat32, fn, ": absmax must be fp32");
  TORCH_CHECK(amax.is_contiguous(), fn, ": absmax must be contiguous");
  TORCH_CHECK(amax.numel() == N * K / block, fn,
              ": absmax must hold N*K/", block, " values");
}

// Returns r (0 without LoRA).  Runs before the lora_scale == 1.0 shortcut
// that hands `t` to the kernel as it came.
static int check_lora(const char* fn, const torch::Tensor& x,
                      const torch::Tensor& t, const torch::Tensor& bw,
                      long M, long N, int r_step, int r_max) {
  if (!(t.defined() && t.numel() > 0)) return 0;
  TORCH_CHECK(t.device() == x.device(), fn, ": t must be on x's device");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": t must be bf16");
  TORCH_CHECK(t.is_contiguous(), fn, ": t must be contiguous");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == M, fn, ": t must be [M, r]");
  const long r = t.size(1);
  TORCH_CHECK(r % r_step == 0 && r <= r_max, fn, ": r must be a multiple of ",
              r_step, ", <= ", r_max);
  TORCH_CHECK(bw.defined() && bw.device() == x.device(), fn,
              ": bw must be on x's device");
  TORCH_CHECK(bw.scalar_type() == torch::kBFloat16, fn, ": bw must be bf16");
  TORCH_CHECK(bw.is_contiguous(), fn, ": bw must be contiguous");
  TORCH_CHECK(bw.dim() == 2 && bw.size(0) == N && bw.size(1) == r, fn,
              ": bw must be [N, r]");
  return (int)r;
}

// Returns the bias pointer, or null for an undefined / empty bias.
static const __hip_bfloat16* check_bias(const char* fn, const torch::Tensor& x,
                                        const torch::Tensor& bias, long N) {
  if (!(bias.defined() && bias.numel() > 0)) return nullptr;
  TORCH_CHECK(bias.device() == x.device(), fn, ": bias must be on x's device");
  TORCH_CHECK(bias.scalar_type() == torch::kBFloat16, fn, ": bias must be bf16");
  TORCH_CHECK(bias.is_contiguous(), fn, ": bias must be contiguous");
  TORCH_CHECK(bias.numel() == N, fn, ": bias must have N elements");
  return (const __hip_bfloat16*)bias.data_ptr();
}

// st_16x32 swizzle on a byte offset within a [rows][64] bf16 image
// (128-B rows): byte bit5 ^= bit9 — spreads each ds_read_b128 lane group
// over four 16-B slots (guide: bank-conflict 141x down, +35%).
DEV_INLINE unsigned swz(unsigned o) { return o ^ (((o >> 9) & 1u) << 5); }

// Stage one [256][64] bf16 tile (32 KB) into `image` via glds: 32 wave-level
// 1-KiB pieces, 4 per wave.  The global source address carries the swizzle;
// rows outside [0, rows_total) are redirected to row 0 (caller guarantees
// alignment so this never happens on the standard path).
DEV_INLINE void stage_tile_glds(__bf16* image, const __hip_bfloat16* gbase,
                                long row0, long ld, int k0, int wave, int lane) {
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) {
    const int piece = wave * 4 + p4;
    const unsigned d = piece * 1024u + lane * 16u;   // LDS dest byte
    const unsigned s = swz(d);                       // source byte in tile
    const int srow = s >> 7;                         // 128-B rows
    const int scol_b = s & 127;
    const __hip_bfloat16* src =
        gbase + (row0 + srow) * ld + k0 + (scol_b >> 1);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// read an A/B fragment (16x16x32 layout: lane -> row l&15, 8 k at (l>>4)*8)
// from a swizzled [.][64] image; `row` relative to the image, k0 in [0,64)
DEV_INLINE bf16x8_g frag_swz(const __bf16* image, int row, int k0) {
  const unsigned o = (unsigned)row * 128u + (unsigned)k0 * 2u;
  return *reinterpret_cast<const bf16x8_g*>((const char*)image + swz(o));
}

__global__ __launch_bounds__(512) void fused_lora_gemm_kernel(
    const __hip_bfloat16* __restrict__ x,   // [M,K]
    const __hip_bfloat16* __restrict__ w,   // [N,K]
    const __hip_bfloat16* __restrict__ t,   // [M,r] or null
    const __hip_bfloat16* __restrict__ bw,  // [N,r] or null
    const __hip_bfloat16* __restrict__ bias,  // [N] or null
    __hip_bfloat16* __restrict__ y,         // [M,N]
    long M, long N, long K, int r, float lora_scale) {
  // one __shared__ array only (glds pipeline rule)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* lds = (__bf16*)smem;  // [2][A 256x64 | B 256x64] = 128 KiB

  // XCD-aware blockIdx remap (guide T1, bijective form): consecutive
  // launch ids land on the same XCD's L2 as neighbors in tile space, so
  // the B tile reused across M-blocks stays resident (+L2 locality on
  // the K>=2048 shapes)
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbn = (int)(N >> 8);
  const int bm = wgid / nbn;
  const int bn = wgid % nbn;
  const long m0 = (long)bm << 8;
  const long n0 = (long)bn << 8;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 2;   // 0..1: wave m-position
  const int wc = wave & 3;    // 0..3: wave n-position
  const int fr = lane & 15;   // fragment row
  const int fq = lane >> 4;   // fragment k-quarter / C row group

  f32x4_g acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_g{0.f, 0.f, 0.f, 0.f};

  __bf16* bufA[2] = {lds, lds + 2 * 256 * 64};
  __bf16* bufB[2] = {lds + 256 * 64, lds + 3 * 256 * 64};

  const int KT = (int)(K >> 6);
  stage_tile_glds(bufA[0], x, m0, K, 0, wave, lane);
  stage_tile_glds(bufB[0], w, n0, K, 0, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) {
      stage_tile_glds(bufA[cur ^ 1], x, m0, K, (kt + 1) << 6, wave, lane);
      stage_tile_glds(bufB[cur ^ 1], w, n0, K, (kt + 1) << 6, wave, lane);
    }
    const __bf16* A = bufA[cur];
    const __bf16* B = bufB[cur];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_g af[8], bf[4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = frag_swz(B, wc * 64 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    // drain next tile's glds, then release the buffers we just read
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- LoRA rank-r epilogue: acc += s * t-tile @ Bw-tile^T ---------------
  if (r > 0) {
    const int RC = r >> 6;  // [256][64] chunks per operand
    // r<=128: both operands fit the 4 buffer slots at once
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_tile_glds(bufA[c & 1], t, m0, r, c << 6, wave, lane);
      stage_tile_glds(bufB[c & 1], bw, n0, r, c << 6, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const __bf16* A = bufA[c & 1];
      const __bf16* B = bufB[c & 1];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_g af[8], bf[4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bf[j] = frag_swz(B, wc * 64 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();
    }
    // fold the LoRA scale: epilogue computed acc_main + t·Bw^T; we need
    // acc_main + s·t·Bw^T.  Instead of scaling inside (would scale the
    // main GEMM too), the host pre-scales t by s — nothing to do here.
  }

  // ---- epilogue: stage each wave's 128x64 tile through its LDS share ----
  // (per-element global stores are store-issue-bound; LDS re-read gives
  // b128 row stores — DESIGN.md rule 6)
  __syncthreads();
  __bf16* mine = lds + wave * (128 * 64);  // 16 KiB per wave
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + fq * 4 + reg;  // within wave tile
        const int col = j * 16 + fr;
        float v = acc[i][j][reg];
        if (bias) v += (float)bias[n0 + wc * 64 + col];
        mine[row * 64 + col] = (__bf16)v;  // writes 2-way (col pairs share a
                                           // dword), reads conflict-free b128
      }
  // no barrier needed: each wave reads only its own region
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (lane >> 3);          // 0..127
    const int cb = (lane & 7) * 8;                 // 8-col chunk
    const bf16x8_g vv = *reinterpret_cast<const bf16x8_g*>(mine + row * 64 + cb);
    *reinterpret_cast<bf16x8_g*>(
        y + (m0 + wr * 128 + row) * N + n0 + wc * 64 + cb) = vv;
  }
}

// ---------------------------------------------------------------------------
// Deep-pipelined variant: 256x128 tile, THREE LDS buffers, counted vmcnt
// with raw s_barrier (the guide's "+83% 3-buf span" glds structure — two
// tiles stay in flight across each barrier; __syncthreads would emit
// vmcnt(0) and drain them, so the K-loop uses __builtin_amdgcn_s_barrier()
// + lgkmcnt(0) only).  A[256x64] + B[128x64] = 48 KiB/buffer, 3 buffers =
// 144 KiB.  8 waves as 2Mx4N -> per-wave 128x32 output (8x2 fragments).
// Targets the K>=2048 shapes where the 2-buffer kernel loses to hipBLASLt.
// ---------------------------------------------------------------------------

// stage a [128][64] bf16 tile (16 KB): 16 pieces, 2 per wave
DEV_INLINE void stage_half_glds(__bf16* image, const __hip_bfloat16* gbase,
                                long row0, long ld, int k0, int wave, int lane) {
#pragma unroll
  for (int p2 = 0; p2 < 2; ++p2) {
    const int piece = wave * 2 + p2;
    const unsigned d = piece * 1024u + lane * 16u;
    const unsigned s = swz(d);
    const int srow = s >> 7;
    const int scol_b = s & 127;
    const __hip_bfloat16* src = gbase + (row0 + srow) * ld + k0 + (scol_b >> 1);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

__global__ __launch_bounds__(512) void fused_lora_gemm3_kernel(
    const __hip_bfloat16* __restrict__ x, const __hip_bfloat16* __restrict__ w,
    const __hip_bfloat16* __restrict__ t, const __hip_bfloat16* __restrict__ bw,
    const __hip_bfloat16* __restrict__ bias, __hip_bfloat16* __restrict__ y,
    long M, long N, long K, int r, float lora_scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* lds = (__bf16*)smem;  // 3 x (A 256x64 + B 128x64) = 144 KiB

  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbn = (int)(N >> 7);
  const int bm = wgid / nbn;
  const int bn = wgid % nbn;
  const long m0 = (long)bm << 8;
  const long n0 = (long)bn << 7;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 2;   // 2 M positions
  const int wc = wave & 3;    // 4 N positions (32 cols each)
  const int fr = lane & 15;
  const int fq = lane >> 4;

  f32x4_g acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_g{0.f, 0.f, 0.f, 0.f};

  __bf16* bufA[3];
  __bf16* bufB[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    bufA[b] = lds + b * (256 * 64 + 128 * 64);
    bufB[b] = bufA[b] + 256 * 64;
  }

  const int KT = (int)(K >> 6);
  // A stage = 8 glds/wave (4 pieces x2 halves... 256x64 = 32KB = 4/wave),
  // B stage = 2/wave; per tile 6 glds/wave.  Keep 2 tiles in flight:
  // wait vmcnt(12) before computing a tile.
  stage_tile_glds(bufA[0], x, m0, K, 0, wave, lane);
  stage_half_glds(bufB[0], w, n0, K, 0, wave, lane);
  if (KT > 1) {
    stage_tile_glds(bufA[1], x, m0, K, 64, wave, lane);
    stage_half_glds(bufB[1], w, n0, K, 64, wave, lane);
  }

  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt % 3;
    if (kt + 2 < KT) {
      const int nxt = (kt + 2) % 3;
      stage_tile_glds(bufA[nxt], x, m0, K, (kt + 2) << 6, wave, lane);
      stage_half_glds(bufB[nxt], w, n0, K, (kt + 2) << 6, wave, lane);
    }
    // tile kt's 6 glds are the oldest; up to 12 newer stay in flight
    if (kt + 2 < KT)
      asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (kt + 1 < KT)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // raw: no vmcnt(0) drain
    const __bf16* A = bufA[cur];
    const __bf16* B = bufB[cur];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_g af[8], bf[2];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bf[j] = frag_swz(B, wc * 32 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // release buffers for re-staging
  }

  // LoRA epilogue (serialized 2-buffer staging; r work is ~r/K of the loop)
  if (r > 0) {
    const int RC = r >> 6;
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_tile_glds(bufA[c & 1], t, m0, r, c << 6, wave, lane);
      stage_half_glds(bufB[c & 1], bw, n0, r, c << 6, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const __bf16* A = bufA[c & 1];
      const __bf16* B = bufB[c & 1];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_g af[8], bf[2];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          bf[j] = frag_swz(B, wc * 32 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  __syncthreads();
  // per-wave 128x32 tile through LDS (16 KiB each within the first 128 KiB)
  __bf16* mine = lds + wave * (128 * 32);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + fq * 4 + reg;
        const int col = j * 16 + fr;
        float v = acc[i][j][reg];
        if (bias) v += (float)bias[n0 + wc * 32 + col];
        mine[row * 32 + col] = (__bf16)v;
      }
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) {
    const int row = rr * 16 + (lane >> 2);
    const int cb = (lane & 3) * 8;
    const bf16x8_g vv = *reinterpret_cast<const bf16x8_g*>(mine + row * 32 + cb);
    *reinterpret_cast<bf16x8_g*>(
        y + (m0 + wr * 128 + row) * N + n0 + wc * 32 + cb) = vv;
  }
}

// ---------------------------------------------------------------------------
// BK=32 / 4-buffer variant: the guide's "3-buffer glds + raw barrier" tier
// (measured 1156-1182 TF at 4k³ there) — counted vmcnt keeps THREE
// sub-tiles of glds in flight across every barrier, so the per-tile
// vmcnt(0) drain that caps the 2-buffer kernel at ~820 TF disappears.
// A[256][32] + B[256][32] = 32 KiB per buffer x 4 = 128 KiB.
// Rows are 64 B here, so the st_16x32 swizzle does not apply; instead the
// 16-B slot rotates by the HIGH row bits (slot ^= (row>>2)&3), which makes
// each 16-lane ds_read_b128 group tile all 64 banks exactly (conflict-free;
// derivation in the comment above swz32).
// ---------------------------------------------------------------------------

// swizzle for [rows][32] bf16 images: byte bit4..5 ^= row bits 2..3
DEV_INLINE unsigned swz32(unsigned o) {
  return o ^ ((((o >> 8) & 3u)) << 4);  // row = o>>6; (row>>2)&3 = (o>>8)&3
}

// stage a [256][32] bf16 sub-tile (16 KB): 16 pieces, 2 per wave
DEV_INLINE void stage_k32_glds(__bf16* image, const __hip_bfloat16* gbase,
                               long row0, long ld, int k0, int wave, int lane) {
#pragma unroll
  for (int p2 = 0; p2 < 2; ++p2) {
    const int piece = wave * 2 + p2;
    const unsigned d = piece * 1024u + lane * 16u;
    const unsigned s = swz32(d);
    const int srow = s >> 6;       // 64-B rows
    const int scol_b = s & 63;
    const __hip_bfloat16* src = gbase + (row0 + srow) * ld + k0 + (scol_b >> 1);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(image) + (piece * 1024u) / 4,
        16, 0, 0);
  }
}

// fragment at (row, k-quarter fq*8): logical byte = row*64 + fq*16
DEV_INLINE bf16x8_g frag_k32q(const __bf16* image, int row, int fq) {
  const unsigned o = (unsigned)row * 64u + (unsigned)fq * 16u;
  return *reinterpret_cast<const bf16x8_g*>((const char*)image + swz32(o));
}

__global__ __launch_bounds__(512) void fused_lora_gemm4_kernel(
    const __hip_bfloat16* __restrict__ x, const __hip_bfloat16* __restrict__ w,
    const __hip_bfloat16* __restrict__ t, const __hip_bfloat16* __restrict__ bw,
    const __hip_bfloat16* __restrict__ bias, __hip_bfloat16* __restrict__ y,
    long M, long N, long K, int r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* lds = (__bf16*)smem;  // 4 x (A 256x32 + B 256x32) = 128 KiB

  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbn = (int)(N >> 8);
  const int bm = wgid / nbn;
  const int bn = wgid % nbn;
  const long m0 = (long)bm << 8;
  const long n0 = (long)bn << 8;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4_g acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_g{0.f, 0.f, 0.f, 0.f};

  __bf16* bufA[4];
  __bf16* bufB[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    bufA[b] = lds + b * (2 * 256 * 32);
    bufB[b] = bufA[b] + 256 * 32;
  }

  const int ST = (int)(K >> 5);  // 32-deep sub-tiles
  // 4 glds per wave per sub-tile (2 A + 2 B); 3 sub-tiles stay in flight
  stage_k32_glds(bufA[0], x, m0, K, 0, wave, lane);
  stage_k32_glds(bufB[0], w, n0, K, 0, wave, lane);
  if (ST > 1) {
    stage_k32_glds(bufA[1], x, m0, K, 32, wave, lane);
    stage_k32_glds(bufB[1], w, n0, K, 32, wave, lane);
  }
  if (ST > 2) {
    stage_k32_glds(bufA[2], x, m0, K, 64, wave, lane);
    stage_k32_glds(bufB[2], w, n0, K, 64, wave, lane);
  }

  for (int s = 0; s < ST; ++s) {
    const int cur = s & 3;
    if (s + 3 < ST) {
      const int nxt = (s + 3) & 3;
      stage_k32_glds(bufA[nxt], x, m0, K, (s + 3) << 5, wave, lane);
      stage_k32_glds(bufB[nxt], w, n0, K, (s + 3) << 5, wave, lane);
    }
    // leave every sub-tile newer than s in flight
    const int ahead = min(3, ST - 1 - s);
    if (ahead >= 3)
      asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (ahead == 2)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // raw: glds stay in flight
    asm volatile("" ::: "memory");  // compiler fence: no read hoists above
    const __bf16* A = bufA[cur];
    const __bf16* B = bufB[cur];
    bf16x8_g af[8], bf[4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      af[i] = frag_k32q(A, wr * 128 + i * 16 + fr, fq);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bf[j] = frag_k32q(B, wc * 64 + j * 16 + fr, fq);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[i], bf[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // buffer release
  }

  // LoRA epilogue: reuse the 2-buffer serialized pattern over 32-deep chunks
  if (r > 0) {
    const int RC = r >> 5;
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_k32_glds(bufA[c & 1], t, m0, r, c << 5, wave, lane);
      stage_k32_glds(bufB[c & 1], bw, n0, r, c << 5, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const __bf16* A = bufA[c & 1];
      const __bf16* B = bufB[c & 1];
      bf16x8_g af[8], bf[4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        af[i] = frag_k32q(A, wr * 128 + i * 16 + fr, fq);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = frag_k32q(B, wc * 64 + j * 16 + fr, fq);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
      __syncthreads();
    }
  }

  __syncthreads();
  __bf16* mine = lds + wave * (128 * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + fq * 4 + reg;
        const int col = j * 16 + fr;
        float v = acc[i][j][reg];
        if (bias) v += (float)bias[n0 + wc * 64 + col];
        mine[row * 64 + col] = (__bf16)v;
      }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (lane >> 3);
    const int cb = (lane & 7) * 8;
    const bf16x8_g vv = *reinterpret_cast<const bf16x8_g*>(mine + row * 64 + cb);
    *reinterpret_cast<bf16x8_g*>(
        y + (m0 + wr * 128 + row) * N + n0 + wc * 64 + cb) = vv;
  }
}


// int8 variant of the dequant stage (256-element symmetric blocks,
// scale = absmax/127 — ops/csrc/quantize.hip layout).  Requires K%256==0
// so each thread's 32-element run stays inside one block.
DEV_INLINE void stage_tile_int8(__bf16* image, const int8_t* qdata,
                                const float* absmax, long row0, long K, int k0,
                                int tid) {
  const int row = tid >> 1;
  const int half = tid & 1;
  const long flat = (row0 + row) * K + k0 + half * 32;
  // absmax / 127, as dequantize_int8 spells it: absmax * (1/127) differs by
  // an fp32 ulp for some blocks, and the forward would then see another W
  // than the backward's materialized one wherever that crosses a bf16 tie
  const float sc = absmax[flat >> 8] / 127.f;
  union { uint32_t u[8]; int8_t b[32]; } pk;
  *reinterpret_cast<uint4*>(pk.u) = *reinterpret_cast<const uint4*>(qdata + flat);
  *reinterpret_cast<uint4*>(pk.u + 4) = *reinterpret_cast<const uint4*>(qdata + flat + 16);
  __bf16 vals[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) vals[i] = (__bf16)(pk.b[i] * sc);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned o = (unsigned)row * 128u + (unsigned)half * 64u + c * 16u;
    *reinterpret_cast<bf16x8_g*>((char*)image + swz(o)) =
        *reinterpret_cast<const bf16x8_g*>(vals + c * 8);
  }
}

__global__ __launch_bounds__(512) void fused_int8_gemm_kernel(
    const __hip_bfloat16* __restrict__ x, const int8_t* __restrict__ qw,
    const float* __restrict__ amax, const __hip_bfloat16* __restrict__ t,
    const __hip_bfloat16* __restrict__ bw, const __hip_bfloat16* __restrict__ bias,
    __hip_bfloat16* __restrict__ y, long M, long N, long K, int r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* lds = (__bf16*)smem;
  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbn = (int)(N >> 8);
  const long m0 = (long)(wgid / nbn) << 8;
  const long n0 = (long)(wgid % nbn) << 8;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  f32x4_g acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_g{0.f, 0.f, 0.f, 0.f};
  __bf16* bufA[2] = {lds, lds + 2 * 256 * 64};
  __bf16* bufB[2] = {lds + 256 * 64, lds + 3 * 256 * 64};
  const int KT = (int)(K >> 6);
  stage_tile_glds(bufA[0], x, m0, K, 0, wave, lane);
  stage_tile_int8(bufB[0], qw, amax, n0, K, 0, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) {
      stage_tile_glds(bufA[cur ^ 1], x, m0, K, (kt + 1) << 6, wave, lane);
      stage_tile_int8(bufB[cur ^ 1], qw, amax, n0, K, (kt + 1) << 6, tid);
    }
    const __bf16* A = bufA[cur];
    const __bf16* B = bufB[cur];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_g af[8], bf[4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = frag_swz(B, wc * 64 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (r > 0) {
    const int RC = r >> 6;
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_tile_glds(bufA[c & 1], t, m0, r, c << 6, wave, lane);
      stage_tile_glds(bufB[c & 1], bw, n0, r, c << 6, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const __bf16* A = bufA[c & 1];
      const __bf16* B = bufB[c & 1];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_g af[8], bf[4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bf[j] = frag_swz(B, wc * 64 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  __syncthreads();
  __bf16* mine = lds + wave * (128 * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + fq * 4 + reg;
        const int col = j * 16 + fr;
        float v = acc[i][j][reg];
        if (bias) v += (float)bias[n0 + wc * 64 + col];
        mine[row * 64 + col] = (__bf16)v;
      }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (lane >> 3);
    const int cb = (lane & 7) * 8;
    const bf16x8_g vv = *reinterpret_cast<const bf16x8_g*>(mine + row * 64 + cb);
    *reinterpret_cast<bf16x8_g*>(
        y + (m0 + wr * 128 + row) * N + n0 + wc * 64 + cb) = vv;
  }
}

torch::Tensor fused_int8_gemm(torch::Tensor x, torch::Tensor qw, torch::Tensor amax,
                              long N, torch::Tensor t, torch::Tensor bw,
                              torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_int8_gemm";
  check_x(fn, x);
  TORCH_CHECK(qw.scalar_type() == torch::kInt8, fn, ": qw must be int8");
  const long M = x.size(0), K = x.size(1);
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 256 == 0,
              "fused_int8_gemm requires M%256==0, N%256==0, K%256==0");
  check_quant_w(fn, x, qw, amax, N, K, N * K, 256);
  const int r = check_lora(fn, x, t, bw, M, N, 64, 256);
  const bool has_lora = r > 0;
  const __hip_bfloat16* bias_p = check_bias(fn, x, bias, N);
  torch::Tensor t_scaled;
  if (has_lora)
    t_scaled = (lora_scale == 1.0) ? t : (t * lora_scale).contiguous();
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((M >> 8) * (N >> 8));
  dim3 block(512);
  size_t smem = 4 * 256 * 64 * sizeof(__bf16);
  hipLaunchKernelGGL(fused_int8_gemm_kernel, grid, block, smem, stream,
                     (const __hip_bfloat16*)x.data_ptr(), (const int8_t*)qw.data_ptr(),
                     amax.data_ptr<float>(),
                     has_lora ? (const __hip_bfloat16*)t_scaled.data_ptr() : nullptr,
                     has_lora ? (const __hip_bfloat16*)bw.data_ptr() : nullptr,
                     bias_p,
                     (__hip_bfloat16*)y.data_ptr(), M, N, K, r);
  HIP_CHECK_LAST();
  return y;
}

// ---------------------------------------------------------------------------
// NF4 variant (K15): the frozen W arrives as packed NF4 (64-element blocks,
// fp32 absmax, hi-nibble = even element — ops/csrc/quantize.hip layout) and
// is dequantized DURING LDS staging, so no dense [N,K] W ever exists in HBM
// (the reference runs bnb matmul_4bit, relora.py:314-317; the round-1 path
// materialized the full dense W per forward — this kernel removes that).
// Same tile structure; B staged by registers (dequant needs a transform,
// which glds cannot do), A stays glds.
// ---------------------------------------------------------------------------

__constant__ float NF4_CODE_G[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f,
    -0.28444138169288635f, -0.18477343022823334f, -0.09105003625154495f, 0.0f,
    0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f,
    0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f,
    0.7229568362236023f, 1.0f};

// stage one [256][64] bf16 B-image from NF4-packed W: thread tid covers
// row = tid/2, elements (tid&1)*32..+32 — one 16-byte packed load + one
// absmax, 32 dequants, 4 swizzled ds_write_b128
DEV_INLINE void stage_tile_nf4(__bf16* image, const uint8_t* qdata,
                               const float* absmax, long row0, long K, int k0,
                               int tid) {
  const int row = tid >> 1;
  const int half = tid & 1;
  const long blk = (row0 + row) * (K >> 6) + (k0 >> 6);
  const float am = absmax[blk];
  const uint8_t* src = qdata + blk * 32 + half * 16;
  union { uint32_t u[4]; uint8_t b[16]; } pk;
  *reinterpret_cast<uint4*>(pk.u) = *reinterpret_cast<const uint4*>(src);
  __bf16 vals[32];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint8_t b = pk.b[i];
    vals[2 * i] = (__bf16)(NF4_CODE_G[b >> 4] * am);
    vals[2 * i + 1] = (__bf16)(NF4_CODE_G[b & 15] * am);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const unsigned o = (unsigned)row * 128u + (unsigned)half * 64u + c * 16u;
    *reinterpret_cast<bf16x8_g*>((char*)image + swz(o)) =
        *reinterpret_cast<const bf16x8_g*>(vals + c * 8);
  }
}

__global__ __launch_bounds__(512) void fused_nf4_gemm_kernel(
    const __hip_bfloat16* __restrict__ x,   // [M,K]
    const uint8_t* __restrict__ qw,         // packed NF4 of W [N,K]
    const float* __restrict__ amax,         // absmax per 64-block
    const __hip_bfloat16* __restrict__ t,   // [M,r] or null (pre-scaled)
    const __hip_bfloat16* __restrict__ bw,  // [N,r] or null
    const __hip_bfloat16* __restrict__ bias,
    __hip_bfloat16* __restrict__ y, long M, long N, long K, int r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* lds = (__bf16*)smem;

  const int nwg = gridDim.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = blockIdx.x;
  if (nwg >= 8) {
    const int xcd = wgid & 7, pos = wgid >> 3;
    wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + pos;
  }
  const int nbn = (int)(N >> 8);
  const int bm = wgid / nbn;
  const int bn = wgid % nbn;
  const long m0 = (long)bm << 8;
  const long n0 = (long)bn << 8;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4_g acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_g{0.f, 0.f, 0.f, 0.f};

  __bf16* bufA[2] = {lds, lds + 2 * 256 * 64};
  __bf16* bufB[2] = {lds + 256 * 64, lds + 3 * 256 * 64};

  const int KT = (int)(K >> 6);
  stage_tile_glds(bufA[0], x, m0, K, 0, wave, lane);
  stage_tile_nf4(bufB[0], qw, amax, n0, K, 0, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) {
      stage_tile_glds(bufA[cur ^ 1], x, m0, K, (kt + 1) << 6, wave, lane);
      stage_tile_nf4(bufB[cur ^ 1], qw, amax, n0, K, (kt + 1) << 6, tid);
    }
    const __bf16* A = bufA[cur];
    const __bf16* B = bufB[cur];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_g af[8], bf[4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bf[j] = frag_swz(B, wc * 64 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  if (r > 0) {
    const int RC = r >> 6;
#pragma unroll 1
    for (int c = 0; c < RC; ++c) {
      stage_tile_glds(bufA[c & 1], t, m0, r, c << 6, wave, lane);
      stage_tile_glds(bufB[c & 1], bw, n0, r, c << 6, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const __bf16* A = bufA[c & 1];
      const __bf16* B = bufB[c & 1];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_g af[8], bf[4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          af[i] = frag_swz(A, wr * 128 + i * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bf[j] = frag_swz(B, wc * 64 + j * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
      __syncthreads();
    }
  }

  __syncthreads();
  __bf16* mine = lds + wave * (128 * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * 16 + fq * 4 + reg;
        const int col = j * 16 + fr;
        float v = acc[i][j][reg];
        if (bias) v += (float)bias[n0 + wc * 64 + col];
        mine[row * 64 + col] = (__bf16)v;
      }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const int row = rr * 8 + (lane >> 3);
    const int cb = (lane & 7) * 8;
    const bf16x8_g vv = *reinterpret_cast<const bf16x8_g*>(mine + row * 64 + cb);
    *reinterpret_cast<bf16x8_g*>(
        y + (m0 + wr * 128 + row) * N + n0 + wc * 64 + cb) = vv;
  }
}

torch::Tensor fused_nf4_gemm(torch::Tensor x, torch::Tensor qw, torch::Tensor amax,
                             long N, torch::Tensor t, torch::Tensor bw,
                             torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_nf4_gemm";
  check_x(fn, x);
  TORCH_CHECK(qw.scalar_type() == torch::kUInt8, fn, ": qw must be uint8");
  const long M = x.size(0), K = x.size(1);
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 64 == 0,
              "fused_nf4_gemm requires M%256==0, N%256==0, K%64==0");
  check_quant_w(fn, x, qw, amax, N, K, N * K / 2, 64);
  const int r = check_lora(fn, x, t, bw, M, N, 64, 256);
  const bool has_lora = r > 0;
  const __hip_bfloat16* bias_p = check_bias(fn, x, bias, N);
  torch::Tensor t_scaled;
  if (has_lora)
    t_scaled = (lora_scale == 1.0) ? t : (t * lora_scale).contiguous();
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((M >> 8) * (N >> 8));
  dim3 block(512);
  size_t smem = 4 * 256 * 64 * sizeof(__bf16);
  hipLaunchKernelGGL(fused_nf4_gemm_kernel, grid, block, smem, stream,
                     (const __hip_bfloat16*)x.data_ptr(), qw.data_ptr<uint8_t>(),
                     amax.data_ptr<float>(),
                     has_lora ? (const __hip_bfloat16*)t_scaled.data_ptr() : nullptr,
                     has_lora ? (const __hip_bfloat16*)bw.data_ptr() : nullptr,
                     bias_p,
                     (__hip_bfloat16*)y.data_ptr(), M, N, K, r);
  HIP_CHECK_LAST();
  return y;
}

torch::Tensor fused_lora_gemm(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                              torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_lora_gemm";
  check_x(fn, x);
  check_dense_w(fn, x, w);
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 64 == 0,
              "fused_lora_gemm requires M%256==0, N%256==0, K%64==0");
  const int r = check_lora(fn, x, t, bw, M, N, 64, 256);
  const bool has_lora = r > 0;
  const __hip_bfloat16* bias_p = check_bias(fn, x, bias, N);
  torch::Tensor t_scaled;
  // fold the LoRA scale into t (bf16 rounding of s*t matches the
  // composed path, which also rounds t·B^T·s contributions in bf16)
  if (has_lora)
    t_scaled = (lora_scale == 1.0) ? t : (t * lora_scale).contiguous();
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  const int nbn = (int)(N >> 8);
  dim3 grid((M >> 8) * nbn);
  dim3 block(512);
  size_t smem = 4 * 256 * 64 * sizeof(__bf16);  // 128 KiB
  hipLaunchKernelGGL(fused_lora_gemm_kernel, grid, block, smem, stream,
                     (const __hip_bfloat16*)x.data_ptr(),
                     (const __hip_bfloat16*)w.data_ptr(),
                     has_lora ? (const __hip_bfloat16*)t_scaled.data_ptr() : nullptr,
                     has_lora ? (const __hip_bfloat16*)bw.data_ptr() : nullptr,
                     bias_p,
                     (__hip_bfloat16*)y.data_ptr(), M, N, K,
                     r, (float)lora_scale);
  HIP_CHECK_LAST();
  return y;
}

torch::Tensor fused_lora_gemm3(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                               torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_lora_gemm3";
  check_x(fn, x);
  check_dense_w(fn, x, w);
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M % 256 == 0 && N % 128 == 0 && K % 64 == 0,
              "fused_lora_gemm3 requires M%256==0, N%128==0, K%64==0");
  const int r = check_lora(fn, x, t, bw, M, N, 64, 128);
  const bool has_lora = r > 0;
  const __hip_bfloat16* bias_p = check_bias(fn, x, bias, N);
  torch::Tensor t_scaled;
  if (has_lora)
    t_scaled = (lora_scale == 1.0) ? t : (t * lora_scale).contiguous();
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((M >> 8) * (N >> 7));
  dim3 block(512);
  size_t smem = 3 * (256 * 64 + 128 * 64) * sizeof(__bf16);  // 144 KiB
  hipLaunchKernelGGL(fused_lora_gemm3_kernel, grid, block, smem, stream,
                     (const __hip_bfloat16*)x.data_ptr(),
                     (const __hip_bfloat16*)w.data_ptr(),
                     has_lora ? (const __hip_bfloat16*)t_scaled.data_ptr() : nullptr,
                     has_lora ? (const __hip_bfloat16*)bw.data_ptr() : nullptr,
                     bias_p,
                     (__hip_bfloat16*)y.data_ptr(), M, N, K,
                     r, (float)lora_scale);
  HIP_CHECK_LAST();
  return y;
}

torch::Tensor fused_lora_gemm4(torch::Tensor x, torch::Tensor w, torch::Tensor t,
                               torch::Tensor bw, torch::Tensor bias, double lora_scale) {
  const char* fn = "fused_lora_gemm4";
  check_x(fn, x);
  check_dense_w(fn, x, w);
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M % 256 == 0 && N % 256 == 0 && K % 32 == 0,
              "fused_lora_gemm4 requires M%256==0, N%256==0, K%32==0");
  const int r = check_lora(fn, x, t, bw, M, N, 32, 256);
  const bool has_lora = r > 0;
  const __hip_bfloat16* bias_p = check_bias(fn, x, bias, N);
  torch::Tensor t_scaled;
  if (has_lora)
    t_scaled = (lora_scale == 1.0) ? t : (t * lora_scale).contiguous();
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::hip::getCurrentHIPStreamMasqueradingAsCUDA();
  dim3 grid((M >> 8) * (N >> 8));
  dim3 block(512);
  size_t smem = 4 * 2 * 256 * 32 * sizeof(__bf16);  // 128 KiB
  hipLaunchKernelGGL(fused_lora_gemm4_kernel, grid, block, smem, stream,
                     (const __hip_bfloat16*)x.data_ptr(),
                     (const __hip_bfloat16*)w.data_ptr(),
                     has_lora ? (const __hip_bfloat16*)t_scaled.data_ptr() : nullptr,
                     has_lora ? (const __hip_bfloat16*)bw.data_ptr() : nullptr,
                     bias_p,
                     (__hip_bfloat16*)y.data_ptr(), M, N, K, r);
  HIP_CHECK_LAST();
  return y;
}
