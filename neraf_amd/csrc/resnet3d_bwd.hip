// ResNet3D scene encoder, backward (train-mode BatchNorm): d loss / d feat[1024] -> gradients of the 43 Conv3d
// weights, the 43 BatchNorm3d affine pairs and (for the cells refreshed this step) of the voxel grid
// (NeRAF_model.py:395-400 keeps that edge alive: "Backprop on vision too", NeRAF_pipeline.py:487).
//
// Every contraction re-uses gemm_f16.hip:
//   dgrad  : dX = dY (*) W^T as the same implicit GEMM with a transposed-convolution loader (tap offsets negated,
//            stride-2 taps filtered by parity), B = weights packed [cin][tap*cout + cout];
//   wgrad  : dW[cout][tap,cin] = sum_m dY[m][cout] X[m@tap][cin] as a "TN" GEMM over the voxels (split-K): both operand tiles
//            are read as they lie in HBM ([voxel][channel] rows, the activation rows shifted by the filter tap) and transposed
//            by the LDS read (ds_read_b64_tr_b16) -- no transposed copies, no im2col;
//   BN     : two passes per layer (per-channel reductions sum dy, sum dy*xhat; then the element-wise dx), with the
//            ReLU mask of the consumer folded into both.
// The gradient chain (dY tensors, dgrad weights, wgrad operands) is fp16 with fp32 accumulation, as the reference's AMP training
// runs it (NeRAF_config.py:79 mixed_precision=True) -- with a power-of-two scale per SCALE GROUP instead of one GradScaler factor:
// BatchNorm backward multiplies by gamma/sigma at every one of the 43 layers, which takes the magnitudes out of fp16's range in
// either direction under any single factor.  A group is the output dY of one BatchNorm backward together with everything the GEMMs
// derive from it before the next BatchNorm backward (its dgrad result, the residual sum): the GEMMs run at ratio 1 and know nothing
// of scales; only the element-wise BatchNorm-backward kernels re-scale (an exact ratio of two powers of two folded into their
// per-channel constant) and only they measure: each records the amax of its output AND of its input, i.e. of the GEMM results of
// the group upstream.  Every tensor of group k is stored as value * S0 * 2^e[k]: S0 from this pass's max|d feat| (exact,
// bwd_prologue_kernel), e[k] from the amax recorded in an EARLIER pass (delayed scaling; the prologue re-centres each group so that
// its amax sits in [2^12, 2^13); recording passes are every 4th, neraf_resnet3d_bwd); every fp32 output is multiplied by
// 1 / (S0 2^e[k]).  A group that overflowed (the recorded amax is the fp32 value before rounding) is re-centred exactly and the
// pass's gradients carry inf -- the GradScaler skips that step like any other overflow; a group whose GEMM results overflowed while
// its producer's output did not is read back as inf by its consumer and steps down by 2^6 per recording pass until it can be
// measured (bwd_prologue_kernel "blind").  The first passes over a workspace are
// calibration passes (repeated until a prologue reports the previous pass clean; exponents are kept relative to the group's input
// so that a correction carries downstream).
// Round 4 ran this chain in bfloat16 (same MFMA rate, 8 significant bits).  Measured (profiles/r05_fp16_chain_ab.txt): the chain's
// own rounding error -- superposition grad(a + b) vs grad(a) + grad(b) through one forward -- 1.2e-2 (median) / 3.0e-2 (worst of 129
// parameter gradients) in bf16, 1.5e-3 / 3.4e-3 in fp16; the gate-matched oracle comparison does not move (4.2e-2 worst either way:
// it is set by the forward's rounding differences amplified through layer3's 64-voxel BatchNorms, not by the gradient chain).
// The bf16 shadows of the activations are gone with the bf16 chain.
#include "resnet3d_common.h"
#include <algorithm>
#include <mutex>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <unordered_map>

namespace {

// ---- packed weights for dgrad: Wt[cin][tap*cout + co] = W[co][cin][tap] ------------------------------------------
// One launch for all convolutions; a workgroup transposes a [32 co][32 cin][taps] brick through LDS: the fp32 source is read in
// contiguous runs of 32*taps floats, the fp16 destination written in 64-byte runs along co.
struct PackTTable {
  int n;
  const float* src[kMaxConv];
  int tile_begin[kMaxConv + 1];                // prefix of (cout/32)*(nrows/32) bricks
  unsigned long long dst_off[kMaxConv];
  int cout[kMaxConv], cin[kMaxConv], taps[kMaxConv], kcols[kMaxConv], nrows[kMaxConv];
};

__global__ __launch_bounds__(256) void pack_dgrad_weights_kernel(PackTTable t, char* __restrict__ packed) {
  extern __shared__ half_t brick[];          // [taps][32 n][34 co]
  int lo = 0, hi = t.n - 1;
  const int bid = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.tile_begin[mid] <= bid) lo = mid; else hi = mid - 1; }
  const int i = lo;
  const int tile = bid - t.tile_begin[i];
  const int n_tiles = t.nrows[i] / 32;
  const int co0 = (tile / n_tiles) * 32, n0 = (tile % n_tiles) * 32;
  const int taps = t.taps[i], cin = t.cin[i], cout = t.cout[i];
  const int run = 32 * taps;
  for (int e = threadIdx.x; e < 32 * run; e += 256) {
    const int co_l = e / run, rem = e - co_l * run;
    const int n_l = rem / taps, tap = rem - n_l * taps;
    float v = 0.f;
    if (n0 + n_l < cin) v = t.src[i][((size_t)(co0 + co_l) * cin + n0) * taps + rem];
    brick[(tap * 32 + n_l) * 34 + co_l] = (half_t)v;
  }
  __syncthreads();
  half_t* dst = reinterpret_cast<half_t*>(packed + t.dst_off[i]);
  const int kc = t.kcols[i];
  for (int e = threadIdx.x; e < 32 * run; e += 256) {
    const int co_l = e & 31, rest = e >> 5;
    const int n_l = rest & 31, tap = rest >> 5;
    dst[(size_t)(n0 + n_l) * kc + tap * cout + co0 + co_l] = brick[(tap * 32 + n_l) * 34 + co_l];
  }
}

int launch_pack_dgrad(neraf_ctx* ctx, const PackTTable& t, int ntiles, int max_taps, char* packed_t, hipStream_t st) {
  const size_t lds = (size_t)max_taps * 32 * 34 * sizeof(half_t);
  static size_t attr_lds = 0;
  if (lds > attr_lds) {
    NERAF_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&pack_dgrad_weights_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_lds = lds;
  }
  hipLaunchKernelGGL(pack_dgrad_weights_kernel, dim3((unsigned)ntiles), dim3(256), lds, st, t, packed_t);
  NERAF_HIP_CHECK(ctx, hipGetLastError());
  return NERAF_OK;
}

// ---- per-tensor scales of the fp16 gradient chain (see the header) ---------------------------------------------------------
constexpr int kChainMax = 64;                  // scale groups per backward (1 + 3 per block + stem = 41): one per lane of one wave
constexpr unsigned kChainMagic = 0x5ca1ab1eu;
constexpr int kChainTarget = 12;               // stored amax is re-centred into [2^12, 2^13): 8x headroom below fp16's 65504
constexpr int kChainOverflowStep = 6;          // a group whose recorded amax is not finite (see bwd_prologue_kernel) steps down by 2^6 per recording pass
struct ChainState {
  unsigned magic;
  unsigned unsettled;                          // groups that, in the last RECORDING pass before the one this prologue opened, overflowed fp16 or
                                               // were computed from an overflowed input (0 in steady state; the calibration loop waits for it)
  unsigned passes;                             // prologues run on this state
  unsigned dfeat_bad;                          // this pass's d feat holds inf / NaN (an overflow upstream: the GradScaler will skip the step)
  unsigned pad[60];
  float pow2[kChainMax];                       // 2^e[t]
  float inv[kChainMax];                        // 1 / (S0 * 2^e[t]): what an fp32 result computed from tensor t is multiplied by
  int e[kChainMax];
};
struct ChainParents { unsigned char p[kChainMax]; };          // the group every group is computed from (ids in production order: p[k] < k)

// ---- BatchNorm backward ----------------------------------------------------------------------------------------
// Both passes work on [rows][64-channel] panels.  Pass 1 reduces sum(dy) and sum(dy*xhat) (registers -> LDS -> one atomic per
// channel per workgroup into a replicated accumulator, see kStatStride); pass 2 writes dx.
struct BnBwdArgs {
  BnSrc s;                    // x (pre-BN), finalised forward statistics, gamma
  const half_t* g16; const float* g32;     // upstream gradient w.r.t. the post-activation tensor (one of them)
  const half_t* act;          // post-activation tensor for the ReLU mask (null = no mask)
  int M, Mpad, C;
  int rows_per_block;         // reduce: rows handled by one workgroup (multiple of 32)
  float* sums; int rep;       // [rep][2][cpad] (replica stride kStatStride): sum dy, sum dy*xhat
  int det;                    // reduce, deterministic mode: row block b STORES its sums into slot b of [slots][2][cpad] (no atomics)
  half_t* dx;                 // apply: gradient w.r.t. the pre-BN conv output [Mpad][C]
  half_t* dy_masked;          // apply (optional): g * (act > 0) for the identity residual branch, re-scaled into group `msc`
  float* dgamma; float* dbeta; const float* inv_scale;   // apply (row-block 0 writes the un-scaled affine gradients): 1 / scale of g
  // scale groups: 2^e of dx's group, of g's group, of the group dy_masked joins (null pointers: no re-scaling); amax_out / amax_in:
  // replicated amax accumulators of dx's group and of g's group (null: this pass does not record)
  const float* osc; const float* isc; const float* msc;
  unsigned* amax_out; unsigned* amax_in;
};

// One thread's 8 channels of a row: the loads (bn_bwd_issue) and their conversion (bn_bwd_finish) are separate so that a kernel can
// have the tile in flight while it still waits for the statistics it needs to use it (every dependent memory round trip of these
// 5-7 us kernels is 1.5-2 us).
struct BnBwdRaw { half8 x; half8 g16; f32x4 g0, g1; half8 act; };
__device__ __forceinline__ void bn_bwd_issue(const BnBwdArgs& p, size_t off, BnBwdRaw& r) {
  r.x = *reinterpret_cast<const half8*>(p.s.x + off);
  if (p.g16) r.g16 = *reinterpret_cast<const half8*>(p.g16 + off);
  else { r.g0 = *reinterpret_cast<const f32x4*>(p.g32 + off); r.g1 = *reinterpret_cast<const f32x4*>(p.g32 + off + 4); }
  if (p.act) r.act = *reinterpret_cast<const half8*>(p.act + off);
}
__device__ __forceinline__ void bn_bwd_finish(const BnBwdArgs& p, const BnBwdRaw& r, float (&xv)[8], float (&g)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) xv[j] = (float)r.x[j];
  if (p.g16) {
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = (float)r.g16[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { g[j] = r.g0[j]; g[4 + j] = r.g1[j]; }
  }
  if (p.act) {
#pragma unroll
    for (int j = 0; j < 8; ++j) if (!((float)r.act[j] > 0.f)) g[j] = 0.f;
  }
}
__device__ __forceinline__ void bn_bwd_load(const BnBwdArgs& p, size_t off, float (&xv)[8], float (&g)[8]) {
  BnBwdRaw r;
  bn_bwd_issue(p, off, r);
  bn_bwd_finish(p, r, xv, g);
}

// grid (row blocks, C / 64)
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BnBwdArgs p) {
  __shared__ float mean[64], rstd[64];
  __shared__ float red[2][32][65];
  const int c_base = blockIdx.y * 64;
  const int tid = threadIdx.x;
  const int ch = tid & 7, rsub = tid >> 3;
  const int r_begin = blockIdx.x * p.rows_per_block;
  const int r_end = min(p.M, r_begin + p.rows_per_block);
  // the first row of this thread is in flight while the forward statistics arrive (two dependent round trips otherwise)
  BnBwdRaw first;
  const bool has_first = r_begin + rsub < r_end;
  if (has_first) bn_bwd_issue(p, (size_t)(r_begin + rsub) * p.C + c_base + ch * 8, first);
  if (tid < 64) { float m, v; bn_mean_var(p.s, c_base + tid, 0.f, m, v); mean[tid] = m; rstd[tid] = rsqrtf(v + 1e-5f); }
  __syncthreads();
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  for (int row = r_begin + rsub; row < r_end; row += 32) {
    float xv[8], g[8];
    if (row == r_begin + rsub) bn_bwd_finish(p, first, xv, g);
    else bn_bwd_load(p, (size_t)row * p.C + c_base + ch * 8, xv, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1[j] += g[j];
      s2[j] += g[j] * (xv[j] - mean[ch * 8 + j]) * rstd[ch * 8 + j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[0][rsub][ch * 8 + j] = s1[j]; red[1][rsub][ch * 8 + j] = s2[j]; }
  __syncthreads();
  if (tid < 128) {
    const int which = tid >> 6, col = tid & 63;
    float acc = 0.f;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) acc += red[which][r][col];
    if (p.det) {
      // slot = first row of the block / 32: the layout the fused dgrad epilogues (GemmParams::stat_det) use for the same buffer
      p.sums[(size_t)(blockIdx.x * (p.rows_per_block >> 5)) * (2 * p.s.cpad) + which * p.s.cpad + c_base + col] = acc;
    } else {
      const int rep = p.rep > 1 ? (blockIdx.x & (p.rep - 1)) * kStatStride : 0;
      atomicAdd(p.sums + rep + which * p.s.cpad + c_base + col, acc);
    }
  }
}

// grid (Mpad / 64, C / 64)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdArgs p) {
  __shared__ float mean[64], rstd[64], k1[64], k2[64], k3[64];
  __shared__ float part[2][4][64];
  const int c_base = blockIdx.y * 64, m0 = blockIdx.x * 64;
  const int tid = threadIdx.x;
  const float inv_m = 1.f / (float)p.M;
  // Everything this workgroup reads is addressed by its block index alone, so all of it is requested up front: its two rows of the
  // tile, the forward statistics and gamma of its 64 channels, the replicas of the two backward sums.  Written in the order they are
  // consumed (sums -> barrier -> statistics -> barrier -> tile) this was three dependent memory round trips in a 7 us kernel.
  BnBwdRaw raw[2];
  size_t offs[2];
  bool in[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = it * 256 + tid, row = e >> 3, ch = e & 7;
    const int m = m0 + row;
    offs[it] = (size_t)m * p.C + c_base + ch * 8;
    in[it] = m < p.M;
    if (in[it]) bn_bwd_issue(p, offs[it], raw[it]);
  }
  float fm = 0.f, fv = 0.f, gam = 0.f;
  // the chain's re-scalings of dx and of the masked copy (wave-uniform scalars, in flight with everything else)
  const float isc = p.isc ? p.isc[0] : 1.f;
  const float rsc = p.osc ? p.osc[0] / isc : 1.f, rmk = p.msc ? p.msc[0] / isc : 1.f;
  if (tid < 64) { bn_mean_var(p.s, c_base + tid, 0.f, fm, fv); gam = p.s.gamma[c_base + tid]; }
  {
    // the replicas of the two sums: four threads per channel take every fourth replica (a chain of rep loads otherwise)
    const int c = c_base + (tid & 63), q = tid >> 6;
    float db = 0.f, dg = 0.f;
    for (int r = q; r < p.rep; r += 4) {          // produced by atomics: read where they executed (stat_ld, resnet3d_common.h)
      db += stat_ld(p.sums + r * kStatStride + c, p.s.read_mode); dg += stat_ld(p.sums + r * kStatStride + p.s.cpad + c, p.s.read_mode);
    }
    part[0][q][tid & 63] = db; part[1][q][tid & 63] = dg;
  }
  __syncthreads();
  if (tid < 64) {
    const int c = c_base + tid;
    const float rs = rsqrtf(fv + 1e-5f);
    const float dbeta = (part[0][0][tid] + part[0][1][tid]) + (part[0][2][tid] + part[0][3][tid]);
    const float dgamma = (part[1][0][tid] + part[1][1][tid]) + (part[1][2][tid] + part[1][3][tid]);
    mean[tid] = fm; rstd[tid] = rs;
    k1[tid] = gam * rs * rsc; k2[tid] = dbeta * inv_m; k3[tid] = dgamma * inv_m;
    if (blockIdx.x == 0 && p.dgamma) { p.dgamma[c] = dgamma * p.inv_scale[0]; p.dbeta[c] = dbeta * p.inv_scale[0]; }
  }
  __syncthreads();
  float am = 0.f, am_in = 0.f;
  half8 o[2], om[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int ch = (it * 256 + tid) & 7;
    if (in[it]) {
      float xv[8], g[8];
      bn_bwd_finish(p, raw[it], xv, g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = ch * 8 + j;
        const float xh = (xv[j] - mean[c]) * rstd[c];
        const float v = k1[c] * (g[j] - k2[c] - xh * k3[c]);
        am = fmaxf(am, fabsf(v));
        am_in = fmaxf(am_in, fabsf(g[j]));
        o[it][j] = (half_t)v;
        om[it][j] = (half_t)(g[j] * rmk);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { o[it][j] = (half_t)0.f; om[it][j] = (half_t)0.f; }
    }
  }
  if (p.amax_out) {
    // recording pass: ONE pair of atomics per workgroup, issued before the tile's stores (their round trip to the memory side
    // overlaps the drain); replicas 256 bytes apart, because same-line atomics serialise there
    __shared__ float wmax[2][4];
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) { am = fmaxf(am, __shfl_xor(am, o2)); am_in = fmaxf(am_in, __shfl_xor(am_in, o2)); }
    if ((tid & 63) == 0) { wmax[0][tid >> 6] = am; wmax[1][tid >> 6] = am_in; }
    __syncthreads();
    if (tid < 2) {
      const float m4 = fmaxf(fmaxf(wmax[tid][0], wmax[tid][1]), fmaxf(wmax[tid][2], wmax[tid][3]));
      unsigned* dst = tid == 0 ? p.amax_out : p.amax_in;
      if (dst && m4 > 0.f) atomicMax(dst + ((blockIdx.x * 3u + blockIdx.y) & (kAmaxRep - 1)) * kAmaxStride, __float_as_uint(m4));
    }
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    *reinterpret_cast<half8*>(p.dx + offs[it]) = o[it];
    if (p.dy_masked) *reinterpret_cast<half8*>(p.dy_masked + offs[it]) = om[it];
  }
}

// ---- pools --------------------------------------------------------------------------------------------------------
// Backward prologue in ONE launch: the power-of-two chain scale S0 from max |d feat| (every workgroup derives the same value from the
// 1024 inputs; workgroup 0 publishes {S0, 1/S0} for the kernels that follow), the average-pool backward
// g[row][c] = d feat[c] * S0 / M, and -- workgroup 0 -- the exponents of the chain's scale groups for THIS pass from the amax recorded
// in the last recording pass (ChainState; group 0 is g itself: e = 0, S0 alone places it).
__global__ __launch_bounds__(256) void bwd_prologue_kernel(const float* __restrict__ dfeat, float* __restrict__ scale, int target_log2, int M,
                                                          int Mpad, int C, half_t* __restrict__ g, ChainState* __restrict__ cs,
                                                          unsigned* __restrict__ amax, int n_groups, ChainParents par) {
  __shared__ float red[4];
  __shared__ unsigned s_am[kChainMax];
  __shared__ ChainParents s_par;
  // workgroup 0 also re-centres the chain (below): everything it reads was written by earlier kernels (the amax words by atomics at
  // the memory side: read there too, like the BatchNorm accumulators, resnet3d_common.h stat_ld) and it sits on the critical path of the
  // whole backward, so all of it is requested up front, together with d feat -- validity is applied to the values afterwards
  constexpr int kWords = kChainMax * kAmaxRep / 256;      // amax words per thread
  unsigned v[kWords];
  unsigned magic = 0u, passes_in = 0u;
  int e_in = 0;
  if (blockIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
      const int i = threadIdx.x + k * 256;
      v[k] = i < n_groups * kAmaxRep ? __hip_atomic_load(amax + (size_t)i * kAmaxStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
    }
    magic = cs->magic; passes_in = cs->passes;
    if ((int)threadIdx.x < n_groups) e_in = cs->e[threadIdx.x];
  }
  float df[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) df[k] = (int)(threadIdx.x + k * 256) < C ? fabsf(dfeat[threadIdx.x + k * 256]) : 0.f;     // C <= 2048
  float m = 0.f;
  int nan_seen = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) { m = (df[k] == df[k] && df[k] > m) ? df[k] : m; nan_seen |= df[k] != df[k]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  const float amx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int es = 0;
  if (amx > 0.f && amx < 3.0e38f) {
    es = target_log2 - (int)floorf(log2f(amx));
    es = es > 100 ? 100 : (es < -100 ? -100 : es);
  }
  const float S = exp2f((float)es);
  if (blockIdx.x == 0) {
    const int dfeat_bad = __syncthreads_or(nan_seen) || !(amx < 3.0e38f);
    if (threadIdx.x == 0) { scale[0] = S; scale[1] = 1.f / S; }
    if ((int)threadIdx.x < kChainMax) { s_par.p[threadIdx.x] = par.p[threadIdx.x]; s_am[threadIdx.x] = 0u; }
    const bool valid = magic == kChainMagic;
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
      const int i = threadIdx.x + k * 256;
      if (i < n_groups * kAmaxRep && v[k]) { amax[(size_t)i * kAmaxStride] = 0u; if (valid) atomicMax(&s_am[i / kAmaxRep], v[k]); any = true; }
    }
    const int recorded = __syncthreads_or(any ? 1 : 0);      // the pass before this one was a recording pass
    if (threadIdx.x < 64) {
      // One wave, lane k = group k.  Exponents are RELATIVE to the group's input (e[k] = e[parent] + d[k]): a group whose own
      // measurement is unusable -- it was computed from an overflowed input, or nothing was recorded -- follows its parent's
      // correction, since a gradient tensor's magnitude is its input's times a per-layer factor.  The recorded amax is the fp32 value
      // BEFORE the fp16 rounding, so an overflowed group is re-centred exactly in one pass.  Both recurrences run down the tree of
      // groups (depth ~40): pointer jumping, six rounds of wave shuffles -- this wave is on the critical path of the whole backward.
      const int lane = threadIdx.x;
      const bool in = lane < n_groups;
      const unsigned mx = in ? s_am[lane] : 0u;
      const int p = (in && lane > 0) ? s_par.p[lane] : 0;
      const int eo = (in && valid) ? e_in : 0;
      const int eo_p = __shfl(eo, p);
      int ok = (lane == 0 || !in) ? 1 : (mx < 0x477fe000u ? 1 : 0);      // 65504.0f: what fp16 can hold
      int anc = p;
#pragma unroll
      for (int r = 0; r < 6; ++r) { ok &= __shfl(ok, anc); anc = __shfl(anc, anc); }      // finite here and in every group upstream
      const int okp = __shfl(ok, p);
      const bool measured = okp && mx > 0u && mx < 0x7f800000u;
      // A group's word merges what its producer recorded (fp32, before rounding: always finite) with what its consumer read back
      // (the fp16 GEMM results derived from it, AFTER rounding): when those overflowed although the producer's output did not, the
      // word reads inf / NaN and says nothing about the magnitude.  Following the parent then would keep the exponent for good if the
      // parent is settled (every later pass inf, the GradScaler skipping every step): such a group steps DOWN by a fixed 2^6 -- an
      // overflow of up to 2^6 x 8 (the headroom) lands inside fp16's range, where the next recording pass measures it exactly; a
      // larger jump takes another step.  It counts as unsettled until a recording pass finds it finite.
      const bool blind = okp && in && lane > 0 && mx >= 0x7f800000u;
      // floor(log2(x)) of a positive finite float is its biased exponent - 127 (a subnormal amax reads as "far too small": it is)
      int done = (lane == 0 || !in || measured || blind) ? 1 : 0;
      int acc = (lane == 0 || !in) ? 0 : (measured ? eo + kChainTarget - ((int)(mx >> 23) - 127) : (blind ? eo - kChainOverflowStep : eo - eo_p));
      int link = done ? lane : p;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const int a2 = __shfl(acc, link), d2 = __shfl(done, link), l2 = __shfl(link, link);
        if (!done) { acc += a2; done = d2; link = l2; }
      }
      const int lim_lo = max(-100, -120 - es), lim_hi = min(100, 120 - es);      // S0 2^e stays a normal float
      const int e = acc < lim_lo ? lim_lo : (acc > lim_hi ? lim_hi : acc);
      const unsigned long long bad = __ballot(in && !ok);
      if (in) { cs->e[lane] = e; cs->pow2[lane] = exp2f((float)e); cs->inv[lane] = exp2f((float)(-es - e)); }
      if (lane == 0) {
        // `unsettled` speaks about the last recording pass; it keeps its value over non-recording passes
        if (!valid) cs->unsettled = (unsigned)n_groups;
        else if (recorded) cs->unsettled = (unsigned)__popcll(bad);
        cs->passes = valid ? passes_in + 1u : 1u;
        cs->dfeat_bad = dfeat_bad ? 1u : 0u;
        cs->magic = kChainMagic;
      }
    }
  }
  const float k = S / (float)M;
  const size_t total = (size_t)Mpad * C;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int row = (int)(idx / C), c = (int)(idx % C);
    g[idx] = (half_t)(row < M ? dfeat[c] * k : 0.f);
  }
}

// maxpool(3,2,1) of relu(bn(x)) backward: g[out voxel] goes to the arg-max input (first maximum), nothing if the max is <= 0.
// Written as a GATHER over the input voxels from the forward's arg-max table: no atomics, no zero fill, fp16 out (the scatter it
// replaced re-evaluated the 27 taps of every window and added fp32 atomics into a zeroed 67 MB buffer: 74 + 10 us).
// An input coordinate i belongs to window o = i/2 through tap d = 0 when i is even, and to windows (i-1)/2 (d = +1) and
// (i+1)/2 (d = -1) when it is odd: at most 8 windows per voxel.
//
// Work is dealt by CELLS of 2 x 2 x 2 input voxels (2c .. 2c+1 per axis): a cell holds one voxel of each parity class -- 1, 2, 2, 2,
// 4, 4, 4 and 8 windows -- so every thread (one cell, 8 channels) does the same 27 compares where a thread per voxel left seven
// lanes in eight waiting for the all-odd one; and all windows its voxels belong to are the 8 windows c .. c+1 per axis, whose
// (arg, g) pairs the thread reads ONCE.  A workgroup owns kGatherCz x kGatherCy x kGatherCx cells and first stages the
// (cz+1)(cy+1)(cx+1) windows they touch in LDS (windows past the last one: arg 255, which equals no tap).  Per voxel the
// contributions are added in the order of the per-voxel gather -- window (i-1)/2 before (i+1)/2 per axis, z outermost, x innermost,
// fp32 from 0, one rounding to fp16 -- so the result is that gather's bit for bit.  Workgroup 0 also writes the zero rows
// [din^3, rows_pad_in).
constexpr int kGatherCz = 2, kGatherCy = 4, kGatherCx = 4;
constexpr int kGatherWin = (kGatherCz + 1) * (kGatherCy + 1) * (kGatherCx + 1);      // 75 windows: 4800 + 9600 bytes
static_assert(kGatherCz * kGatherCy * kGatherCx * 8 == 256, "one cell-chunk per thread");

inline unsigned gather_blocks(int din) {
  const int nc = (din + 1) / 2;
  return (unsigned)(((nc + kGatherCz - 1) / kGatherCz) * ((nc + kGatherCy - 1) / kGatherCy) * ((nc + kGatherCx - 1) / kGatherCx));
}

__global__ __launch_bounds__(256) void maxpool_bwd_gather_kernel(const unsigned char* __restrict__ arg, int din, int dout,
                                                                const half_t* __restrict__ g, half_t* __restrict__ dpost, size_t rows_pad_in) {
  __shared__ unsigned long long s_arg[kGatherWin * 8];
  __shared__ uint4 s_g[kGatherWin * 8];
  const int tid = threadIdx.x;
  const int nc = (din + 1) / 2;
  const int nbx = (nc + kGatherCx - 1) / kGatherCx, nby = (nc + kGatherCy - 1) / kGatherCy;
  const int bx = blockIdx.x % nbx, by = (blockIdx.x / nbx) % nby, bz = blockIdx.x / (nbx * nby);
  const int oz0 = bz * kGatherCz, oy0 = by * kGatherCy, ox0 = bx * kGatherCx;
  {
    // all requests of the thread before the first LDS write; windows past the end are read at the clamped coordinate (no branch
    // between the requests) and replaced
    constexpr int kSt = (kGatherWin * 8 + 255) / 256;
    unsigned long long am_s[kSt]; uint4 g_s[kSt]; bool inside[kSt];
#pragma unroll
    for (int k = 0; k < kSt; ++k) {
      const int e = min(k * 256 + tid, kGatherWin * 8 - 1);
      const int w = e >> 3;
      const int oz = oz0 + w / ((kGatherCx + 1) * (kGatherCy + 1)), oy = oy0 + (w / (kGatherCx + 1)) % (kGatherCy + 1), ox = ox0 + w % (kGatherCx + 1);
      inside[k] = oz < dout && oy < dout && ox < dout;
      const size_t ov = ((size_t)min(oz, dout - 1) * dout + min(oy, dout - 1)) * dout + min(ox, dout - 1);
      am_s[k] = *reinterpret_cast<const unsigned long long*>(arg + ov * 64 + (e & 7) * 8);
      g_s[k] = *reinterpret_cast<const uint4*>(g + ov * 64 + (e & 7) * 8);
    }
#pragma unroll
    for (int k = 0; k < kSt; ++k) {
      const int e = k * 256 + tid;
      if (e < kGatherWin * 8) { s_arg[e] = inside[k] ? am_s[k] : ~0ull; s_g[e] = inside[k] ? g_s[k] : make_uint4(0u, 0u, 0u, 0u); }
    }
  }
  if (blockIdx.x == 0) {
    const size_t first = cube(din) * 8, total = rows_pad_in * 8;
    for (size_t e = first + tid; e < total; e += 256) reinterpret_cast<uint4*>(dpost)[e] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  const int ch = tid & 7, lc = tid >> 3;
  const int lx = lc % kGatherCx, ly = (lc / kGatherCx) % kGatherCy, lz = lc / (kGatherCx * kGatherCy);
  unsigned long long am[8];
  half8 gv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int w = ((lz + (k >> 2)) * (kGatherCy + 1) + ly + ((k >> 1) & 1)) * (kGatherCx + 1) + lx + (k & 1);
    am[k] = s_arg[w * 8 + ch];
    const uint4 raw = s_g[w * 8 + ch];
    gv[k] = *reinterpret_cast<const half8*>(&raw);
  }
  // a voxel of parity p on an axis: p = 0 -> window offset 0 through tap 1; p = 1 -> offset 0 through tap 2 (d = +1), then offset 1
  // through tap 0 (d = -1)
#pragma unroll
  for (int pz = 0; pz < 2; ++pz)
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int iz = 2 * (oz0 + lz) + pz, iy = 2 * (oy0 + ly) + py, ix = 2 * (ox0 + lx) + px;
        if (iz >= din || iy >= din || ix >= din) continue;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int a = 0; a <= pz; ++a)
#pragma unroll
          for (int b = 0; b <= py; ++b)
#pragma unroll
            for (int c = 0; c <= px; ++c) {
              const unsigned tap = (unsigned)((pz ? 2 - 2 * a : 1) * 9 + (py ? 2 - 2 * b : 1) * 3 + (px ? 2 - 2 * c : 1));
              const int k = a * 4 + b * 2 + c;
#pragma unroll
              for (int j = 0; j < 8; ++j)
                if (((am[k] >> (8 * j)) & 0xffu) == tap) acc[j] += (float)gv[k][j];
            }
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)acc[j];      // at most 8 windows meet in a voxel: inside the group's headroom, and measured by the consumer
        *reinterpret_cast<half8*>(dpost + (((size_t)iz * din + iy) * din + ix) * 64 + ch * 8) = o;
      }
}

__global__ void set_f32x2_kernel(float* p, float a, float b) { if (threadIdx.x == 0 && blockIdx.x == 0) { p[0] = a; p[1] = b; } }
__global__ void set_u64_kernel(unsigned long long* p, unsigned long long v) { if (threadIdx.x == 0 && blockIdx.x == 0) p[0] = v; }

// stem input gradient for a window of cells: dgrid[c][cell] = sum_taps sum_co dY[(z+2-dz)/2,...][co] W[co][c][tap] / S.
// One wave per cell, lanes over the 64 output channels; the weights are read as Wt[tap][c][co] fp32 (every load one coalesced row;
// W[co][c][tap] would cost 64 cache lines per load instruction), a layout the backward's weight-pack launch writes into the stem's
// slot of the packed blob (stem_wt_relayout below; the stem has no dgrad GEMM, so the slot is otherwise unused).
__global__ __launch_bounds__(256) void stem_w_relayout_kernel(const float* __restrict__ W, float* __restrict__ Wt) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < kStemWtElems) stem_wt_relayout(W, Wt, idx);
}

// The taps that reach a cell are known from its parity: per axis dz = t0 + 2 j with t0 = (z + pad) & 1 = z & 1, j = 0 .. 2 - t0, from
// source voxel ((z + 2 - t0) >> 1) - j.  All 27 (jz, jy, jx) are walked without a branch: coordinates are clamped into the tensor
// and the table, every dY row of the cell is requested before the first FMA and the weights a z-plane (63 rows) at a time, and a
// tap outside the filter or the tensor leaves the accumulators as they are (a select on a wave-uniform flag).  The reaching taps
// are added in ascending (dz, dy, dx) order, one FMA chain per lane and channel, then the 64 lanes by shuffles: the order -- and
// so every bit -- of the per-tap loop this replaces (one dependent dY load and seven dependent weight loads per reaching tap).
__global__ __launch_bounds__(256) void stem_dgrid_kernel(const half_t* __restrict__ dy, const float* __restrict__ Wt, int S, int dout,
                                                        const unsigned long long* __restrict__ start_dev, int n, int nch,
                                                        const float* __restrict__ inv_scale, float* __restrict__ dgrid) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const size_t cell = (size_t)start_dev[0] + i;   // device-side so that the captured launch sequence does not depend on the window
  const int x = (int)(cell % S), y = (int)((cell / S) % S), z = (int)(cell / ((size_t)S * S));
  const int t0z = z & 1, t0y = y & 1, t0x = x & 1;
  const int bz = (z + 2 - t0z) >> 1, by = (y + 2 - t0y) >> 1, bx = (x + 2 - t0x) >> 1;
  bool okz[3], oky[3], okx[3];
  int sz[3], sy[3], sx[3], tz[3], ty[3], tx[3];            // clamped source coordinate and clamped tap index per axis
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int az = bz - j, ay = by - j, ax = bx - j;
    okz[j] = t0z + 2 * j < 5 && az >= 0 && az < dout; oky[j] = t0y + 2 * j < 5 && ay >= 0 && ay < dout; okx[j] = t0x + 2 * j < 5 && ax >= 0 && ax < dout;
    sz[j] = min(max(az, 0), dout - 1); sy[j] = min(max(ay, 0), dout - 1); sx[j] = min(max(ax, 0), dout - 1);
    tz[j] = min(t0z + 2 * j, 4); ty[j] = min(t0y + 2 * j, 4); tx[j] = min(t0x + 2 * j, 4);
  }
  half_t d[27];
#pragma unroll
  for (int jz = 0; jz < 3; ++jz)
#pragma unroll
    for (int jy = 0; jy < 3; ++jy)
#pragma unroll
      for (int jx = 0; jx < 3; ++jx)
        d[(jz * 3 + jy) * 3 + jx] = dy[((size_t)(sz[jz] * dout + sy[jy]) * dout + sx[jx]) * 64 + lane];
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jz = 0; jz < 3; ++jz) {
    float w[9][7];
#pragma unroll
    for (int jy = 0; jy < 3; ++jy)
#pragma unroll
      for (int jx = 0; jx < 3; ++jx) {
        const float* wp = Wt + (size_t)((tz[jz] * 5 + ty[jy]) * 5 + tx[jx]) * 512 + lane;
#pragma unroll
        for (int c = 0; c < 7; ++c) w[jy * 3 + jx][c] = wp[c * 64];
      }
#pragma unroll
    for (int jy = 0; jy < 3; ++jy)
#pragma unroll
      for (int jx = 0; jx < 3; ++jx) {
        const bool ok = okz[jz] && oky[jy] && okx[jx];
        const float dv = (float)d[(jz * 3 + jy) * 3 + jx];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          const float a = fmaf(dv, w[jy * 3 + jx][c], acc[c]);
          acc[c] = (ok && c < nch) ? a : acc[c];
        }
      }
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    if (c >= nch) break;
    float v = acc[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) dgrid[(size_t)c * n + i] = v * inv_scale[0];
  }
}

__global__ void f16_to_f32_kernel(const half_t* __restrict__ a, size_t n, const float* __restrict__ mul, float* __restrict__ o) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = (float)a[i] * mul[0];
}

// ---- backward workspace ---------------------------------------------------------------------------------------------
struct BwdLayout {
  size_t wt[64];              // dgrad weights (in the packed-dgrad blob)
  size_t packed_total;
  size_t scale;               // fp32[4]
  size_t chain, amax;         // ChainState; replicated amax accumulators [kChainMax][kAmaxRep] words, kAmaxStride words apart
  size_t sums[64];            // per conv/BN: [rep][2][cpad] fp32 (replica stride kStatStride); deterministic mode: [slots][2][cpad]
  size_t sums_fin[64];        // deterministic mode: the slots added in a fixed order, [2][cpad] (what bn_bwd_apply reads)
  size_t sums_begin, sums_bytes;
  size_t g[2];                // ping-pong gradient w.r.t. block outputs, fp16, largest activation
  size_t dy[64];              // dY of every convolution [rows_pad(dout)][cout] fp16: all alive until the grouped weight-gradient launch
  size_t gm, da;              // masked g (identity residual), d(a1|a2) scratch
  size_t dpost;               // fp32 [din1^3][64] stem
  size_t wtmp;                // 256 KB no launch uses any more (the stem's Wt table moved into the packed blob); the offsets after it stay put
  size_t splitk; size_t splitk_bytes;
  size_t total;
};

// row blocks / accumulator replicas of the BN-backward reduction of conv ci
inline int bwd_rows_per_block(const ConvSpec& c) {
  static const int min_rows = [] { const char* e = getenv("NERAF_BN_BWD_MIN_ROWS"); return e ? atoi(e) : 32; }();
  static const int max_blocks = [] { const char* e = getenv("NERAF_BN_BWD_MAX_BLOCKS"); return e ? atoi(e) : 512; }();
  const int M = (int)cube(c.dout);
  return std::max(min_rows, round_up((M + max_blocks - 1) / max_blocks, 32));
}
inline int bwd_stat_rep(const ConvSpec& c) {
  if (2 * round_up(c.cout, 128) > kStatStride) return 1;
  const int M = (int)cube(c.dout), rpb = bwd_rows_per_block(c);
  const int nrb = (M + rpb - 1) / rpb;
  int r = 1;
  while (r < 16 && r * 8 < nrb) r <<= 1;
  return r;
}

void make_bwd_layout(const Arch& A, BwdLayout* L) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += round_up_sz(bytes, 256); return o; };
  for (int i = 0; i < A.nconv; ++i) {
    const ConvSpec& c = A.conv[i];
    const int nrows = c.cin == 64 || c.cin == 8 ? 64 : round_up(c.cin, 128);
    L->wt[i] = take((size_t)nrows * c.k * c.k * c.k * c.cout * 2);
  }
  L->packed_total = off;
  off = 0;
  L->scale = take(256);
  L->chain = take(sizeof(ChainState));
  L->amax = take((size_t)kChainMax * kAmaxRep * kAmaxStride * 4);
  L->sums_begin = off;
  for (int i = 0; i < A.nconv; ++i) {
    const int rep = bwd_stat_rep(A.conv[i]);
    if (neraf_deterministic()) L->sums[i] = take(det_slots(A.conv[i]) * 2 * round_up(A.conv[i].cout, 128) * 4);
    else L->sums[i] = take(rep > 1 ? (size_t)rep * kStatStride * 4 : (size_t)2 * round_up(A.conv[i].cout, 128) * 4);
  }
  L->sums_bytes = off - L->sums_begin;
  for (int i = 0; i < A.nconv; ++i) L->sums_fin[i] = take((size_t)2 * round_up(A.conv[i].cout, 128) * 4);
  size_t max_act = 0, max_wtmp = 0;
  for (int i = 0; i < A.nconv; ++i) {
    const ConvSpec& c = A.conv[i];
    const size_t rows_out = rows_pad(c.dout), rows_in = rows_pad(c.din);
    if (i > 0) {
      max_act = std::max(max_act, rows_out * c.cout * 2);
      max_act = std::max(max_act, rows_in * c.cin * 2);
    }
    max_wtmp = std::max(max_wtmp, (size_t)125 * 8 * 64 * 4);
  }
  for (int i = 0; i < 2; ++i) L->g[i] = take(max_act);
  for (int i = 0; i < A.nconv; ++i) L->dy[i] = take(rows_pad(A.conv[i].dout) * A.conv[i].cout * 2);
  L->gm = take(max_act); L->da = take(max_act);
  L->dpost = take(cube(A.conv[0].dout) * 64 * 4);
  L->wtmp = take(max_wtmp);
  L->splitk_bytes = (size_t)192 << 20;      // K-split slabs of the weight-gradient launch + one slab per un-split filter with taps
  L->splitk = take(L->splitk_bytes);
  L->total = off;
}

struct Ctx {
  neraf_ctx* ctx; hipStream_t st; const Arch* A; const Layout* L; const BwdLayout* B;
  const char* packed_t; char* ws; char* bws; const float* const* bn; float* const* w_grads; float* const* bn_grads;
  // scale group k of the fp16 chain: its 2^e, its 1 / (S0 2^e), its amax accumulator
  const float* pow2(int t) const { return reinterpret_cast<const ChainState*>(bws + B->chain)->pow2 + t; }
  const float* inv(int t) const { return reinterpret_cast<const ChainState*>(bws + B->chain)->inv + t; }
  const float* inv_base() const { return reinterpret_cast<const ChainState*>(bws + B->chain)->inv; }
  bool track = true;          // false: producers do not record amax (NERAF_CHAIN_AMAX=0, measurement only: the scales stay where they are)
  unsigned* amax(int t) const { return track ? reinterpret_cast<unsigned*>(bws + B->amax) + (size_t)t * kAmaxRep * kAmaxStride : nullptr; }
};

// BN backward of conv ci: gradient w.r.t. the conv output, into `dx`
// k_in / k_out: scale groups of g and of dx; k_mask: the group dy_masked joins (the residual sum it is added into)
int bn_backward(const Ctx& c, int ci, const half_t* g16, const float* g32, const half_t* act, half_t* dx, half_t* dy_masked,
                int k_in, int k_out, int k_mask, bool sums_done = false) {
  const ConvSpec& cs = c.A->conv[ci];
  BnBwdArgs p{};
  p.s = bn_src_bwd(*c.A, *c.L, c.ws, c.bn, ci);
  p.g16 = g16; p.g32 = g32; p.act = act;
  p.M = (int)cube(cs.dout); p.Mpad = (int)rows_pad(cs.dout); p.C = cs.cout;
  p.rows_per_block = bwd_rows_per_block(cs);
  p.sums = (float*)(c.bws + c.B->sums[ci]); p.rep = bwd_stat_rep(cs);
  p.dx = dx; p.dy_masked = dy_masked;
  p.dgamma = c.bn_grads[2 * ci]; p.dbeta = c.bn_grads[2 * ci + 1]; p.inv_scale = c.inv(k_in);
  p.osc = c.pow2(k_out); p.isc = c.pow2(k_in); p.msc = dy_masked ? c.pow2(k_mask) : nullptr;
  p.amax_out = c.amax(k_out); p.amax_in = g16 ? c.amax(k_in) : nullptr;
  const int nrb = (p.M + p.rows_per_block - 1) / p.rows_per_block;
  p.det = neraf_deterministic() ? 1 : 0;
  // sums_done: the dgrad GEMM that produced g16 already reduced sum g and sum g * xhat in its epilogue (fuse_bn_sums below)
  if (!sums_done) hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nrb, p.C / 64), dim3(256), 0, c.st, p);
  if (c.ctx && c.ctx->manifest) {
    char nm[96];
    const double elems = (double)p.M * p.C;
    if (!sums_done) {
      snprintf(nm, sizeof(nm), "bn_bwd_reduce_kernel | M=%d C=%d", p.M, p.C);
      neraf_node(c.ctx, nm, 0.0, elems * (2.0 + (g16 ? 2.0 : 4.0) + (act ? 2.0 : 0.0)), 0.0);
    }
    snprintf(nm, sizeof(nm), "bn_bwd_apply_kernel | M=%d C=%d%s", p.M, p.C, dy_masked ? " + masked copy" : "");
    neraf_node(c.ctx, nm, 0.0, elems * (2.0 + (g16 ? 2.0 : 4.0) + (act ? 2.0 : 0.0)), (double)p.Mpad * p.C * 2.0 * (dy_masked ? 2 : 1));
  }
  static const int skip_small = [] { const char* e = getenv("NERAF_SKIP_SMALL_BN"); return e ? atoi(e) : 0; }();      // measurement only, see resnet3d.hip
  if (skip_small >= 2 && cube(cs.dout) <= 4096 && cs.k == 1) return NERAF_OK;     // BatchNorms of 1x1x1 convolutions: their dgrad consumer is a plain GEMM
  if (p.det) {     // the slots (of the reduce kernel or of the fused epilogue) added in a fixed order; the apply pass reads that
    float* fin = (float*)(c.bws + c.B->sums_fin[ci]);
    run_slot_sum(c.st, p.sums, det_slots(cs), p.s.cpad, 0.f, 0, fin);
    p.sums = fin; p.rep = 1;
  }
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(p.Mpad / 64, p.C / 64), dim3(256), 0, c.st, p);
  NERAF_HIP_CHECK(c.ctx, hipGetLastError());
  return NERAF_OK;
}

inline WgradItem wgrad_item(const Ctx& c, int ci, const half_t* dy, const half_t* x_in, int t_dy) {
  const ConvSpec& cs = c.A->conv[ci];
  WgradItem it{};
  it.dy = dy; it.x = x_in; it.out = c.w_grads[ci];
  it.cout = cs.cout; it.cin = cs.cin; it.cin_real = cs.cin_real; it.ksize = cs.k; it.stride = cs.stride; it.pad = cs.pad;
  it.din = cs.din; it.dout = cs.dout; it.K = (int)rows_pad(cs.dout);
  it.alpha_idx = t_dy;
  return it;
}

// dW of ONE conv (the stage test entry); the network's backward collects all items and launches them together
int conv_wgrad(const Ctx& c, int ci, const half_t* dy, const half_t* x_in, int t_dy) {
  const WgradItem it = wgrad_item(c, ci, dy, x_in, t_dy);
  return launch_wgrad_grouped(c.ctx, &it, 1, (const half_t*)(c.ws + c.L->zero_page), (float*)(c.bws + c.B->splitk), c.B->splitk_bytes,
                              c.inv_base(), c.st);
}

// The BatchNorm-backward reduction of the layer that CONSUMES a dgrad's result, folded into that dgrad's epilogue (or split-K
// reducer): for the <= 4096-voxel layers bn_bwd_reduce_kernel is a 3-4 us launch around a few hundred KB, 26 of them per backward.
// NERAF_BN_FUSE_SUMS=0 restores the separate launches.
inline bool fuse_bn_sums(const ConvSpec& bn_conv) {
  static const int on = [] { const char* e = getenv("NERAF_BN_FUSE_SUMS"); return e ? atoi(e) : 1; }();
  static const long max_vox = [] { const char* e = getenv("NERAF_BN_FUSE_MAX_VOX"); return e ? atol(e) : 4096l; }();      // A/B knob
  return on && (long)cube(bn_conv.dout) <= max_vox && (bn_conv.cout % 64) == 0;
}

// the stem is the 7 -> 64 channel 5x5x5 convolution stem_dgrid_kernel is written for: its Wt table is part of the packed blob
inline bool stem_wt_packed(const Arch& A) { return A.conv[0].k == 5 && A.conv[0].cin_real == 7 && A.conv[0].cout == 64; }

// dX [din^3][cin] = conv_transpose(dY [dout^3][cout], W) (+ add16).  bn_ci >= 0: the result is the gradient w.r.t. relu(bn_{bn_ci}(.))
// (+ residual), `bn_act` that post-activation tensor: the epilogue masks the result with it and reduces the two
// BatchNorm-backward sums of conv bn_ci into its accumulators.  The result (and add16) live in dy's scale group: ratio 1.
int conv_dgrad(const Ctx& c, int ci, const half_t* dy, const half_t* add16, half_t* dx, int bn_ci = -1, const half_t* bn_act = nullptr) {
  const ConvSpec& cs = c.A->conv[ci];
  GemmParams g{};
  const int taps = cs.k * cs.k * cs.k;
  g.A = (const half_t*)dy; g.lda = cs.cout;
  g.B = (const half_t*)(c.packed_t + c.B->wt[ci]); g.ldb = taps * cs.cout;
  g.M = (int)cube(cs.din); g.N = cs.cin; g.K = taps * cs.cout; g.Mpad = (int)rows_pad(cs.din);
  g.Npad = cs.cin == 64 ? 64 : round_up(cs.cin, 128); g.tile_n = cs.cin == 64 ? 64 : 0; g.alpha = 1.f;
  g.alg_flops = 2.0 * (double)cube(cs.dout) * taps * cs.cin_real * cs.cout;      // the transposed conv has the forward's MAC count
  g.add16 = (const half_t*)add16; g.ldadd = cs.cin;
  g.C16 = (half_t*)dx; g.ldc16 = cs.cin;
  g.splitk_ws = (float*)(c.bws + c.B->splitk); g.splitk_ws_bytes = c.B->splitk_bytes;
  if (bn_ci >= 0) {
    const ConvSpec& bs = c.A->conv[bn_ci];        // bs.cout == cs.cin, cube(bs.dout) == cube(cs.din)
    float* sums = (float*)(c.bws + c.B->sums[bn_ci]);
    g.colsum = sums; g.colsumsq = sums + round_up(bs.cout, 128);
    g.stat_rep = bwd_stat_rep(bs); g.stat_stride = kStatStride;
    if (neraf_deterministic()) { g.stat_det = 1; g.stat_rep = 0; g.stat_stride = 2 * round_up(bs.cout, 128); }
    g.bnb_x = (const half_t*)(c.ws + c.L->pre[bn_ci]); g.ldbnb = bs.cout; g.bnb_mask = (const half_t*)bn_act;
    g.bnb_fin = (const float*)(c.ws + c.L->fin[bn_ci]); g.bnb_cpad = round_up(bs.cout, 128);
  }
  if (cs.k == 1 && cs.stride == 1) {
    g.conv.loader = 0;
  } else {
    g.conv.loader = 1; g.conv.cin = cs.cout; g.conv.din = cs.dout; g.conv.dout = cs.din; g.conv.stride = 1; g.conv.pad = -cs.pad;
    g.conv.ksize = cs.k; g.conv.tflip = 1; g.conv.tstride = cs.stride;
    g.conv.zero_page = (const half_t*)(c.ws + c.L->zero_page);
  }
  return launch_gemm_f16(c.ctx, g, c.st);
}

}  // namespace

// =================================================================================================
extern "C" size_t neraf_resnet3d_bwd_packed_bytes(const neraf_resnet3d_desc* d) {
  Arch A; BwdLayout B;
  if (make_arch(d, &A)) return 0;
  make_bwd_layout(A, &B);
  return B.packed_total;
}

extern "C" size_t neraf_resnet3d_bwd_workspace_bytes(const neraf_resnet3d_desc* d) {
  Arch A; BwdLayout B;
  if (make_arch(d, &A)) return 0;
  make_bwd_layout(A, &B);
  return B.total;
}

extern "C" int neraf_resnet3d_pack_weights_bwd(neraf_ctx* ctx, const neraf_resnet3d_desc* d, const float* const* conv_w, void* packed_t,
                                               neraf_stream_t stream) {
  Arch A; BwdLayout B;
  if (make_arch(d, &A) || !conv_w || !packed_t) return neraf_fail(ctx, NERAF_EINVAL, "resnet3d_pack_weights_bwd: bad arguments");
  make_bwd_layout(A, &B);
  hipStream_t st = (hipStream_t)stream;
  PackTTable t{};
  BrickTable bt{};
  int acc = 0, max_taps = 1, tiles = 0, max_run = 0;
  for (int i = 1; i < A.nconv; ++i) {            // the stem has no dgrad GEMM (its input gradient is stem_dgrid_kernel's)
    const ConvSpec& c = A.conv[i];
    const int taps = c.k * c.k * c.k;
    const int nrows = c.cin == 64 || c.cin == 8 ? 64 : round_up(c.cin, 128);
    if (brick_packable(c) && nrows == c.cin) {
      const int j = bt.n++;
      int cob, cib;
      brick_shape(c, 1, &cob, &cib);
      bt.src[j] = conv_w[i]; bt.tile_begin[j] = tiles; bt.dst_off[j] = B.wt[i];
      bt.cout[j] = c.cout; bt.cin[j] = c.cin; bt.taps[j] = taps; bt.cib[j] = cib; bt.cob[j] = cob;
      tiles += (c.cout / cob) * (c.cin / cib);
      max_run = std::max(max_run, cob * (cib * taps + 2));
      continue;
    }
    const int j = t.n++;
    t.src[j] = conv_w[i]; t.tile_begin[j] = acc; t.dst_off[j] = B.wt[i];
    t.cout[j] = c.cout; t.cin[j] = c.cin_real; t.taps[j] = taps; t.kcols[j] = taps * c.cout; t.nrows[j] = nrows;
    acc += (c.cout / 32) * (nrows / 32);
    max_taps = std::max(max_taps, taps);
  }
  t.tile_begin[t.n] = acc;
  bt.tile_begin[bt.n] = tiles;
  if (t.n > 0)
    if (int e = launch_pack_dgrad(ctx, t, acc, max_taps, (char*)packed_t, st)) return e;
  // the stem's fp32 Wt[tap][c][co] for stem_dgrid_kernel, in the stem's (otherwise unused) slot of the blob: extra workgroups of
  // the brick launch, or a launch of its own where no convolution takes the brick packer
  const bool stem_wt = stem_wt_packed(A);
  if (stem_wt && bt.n == 0) {
    hipLaunchKernelGGL(stem_w_relayout_kernel, dim3((kStemWtElems + 255) / 256), dim3(256), 0, st, conv_w[0], (float*)((char*)packed_t + B.wt[0]));
    NERAF_HIP_CHECK(ctx, hipGetLastError());
  }
  if (bt.n > 0) {
    if (stem_wt) { bt.stem_w = conv_w[0]; bt.stem_off = B.wt[0]; tiles += (kStemWtElems + 1023) / 1024; }
    const size_t lds = brick_lds_bytes(max_run);
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
      NERAF_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&pack_bricks_kernel<1>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      attr_lds = lds;
    }
    hipLaunchKernelGGL(pack_bricks_kernel<1>, dim3((unsigned)tiles), dim3(256), lds, st, bt, (char*)packed_t);
    NERAF_HIP_CHECK(ctx, hipGetLastError());
  }
  return NERAF_OK;
}

static int resnet3d_bwd_body(neraf_ctx* ctx, const Arch& A, const Layout& L, const BwdLayout& B, const void* packed_t,
                             const float* const* conv_w, const float* const* bn, char* ws, char* bws, const float* dfeat,
                             float* const* w_grads, float* const* bn_grads, int n_cells, int n_ch, float* dgrid_cells, hipStream_t st,
                             bool track) {
  float* scale = (float*)(bws + B.scale);
  neraf_zero_async(st, bws + B.sums_begin, B.sums_bytes);
  neraf_node(ctx, "neraf_zero_kernel | BatchNorm-backward accumulators", 0.0, 0.0, (double)B.sums_bytes);
  const int Mlast = (int)cube(A.final_edge);
  Ctx c{ctx, st, &A, &L, &B, (const char*)packed_t, ws, bws, bn, w_grads, bn_grads};
  c.track = track;
  half_t* g = (half_t*)(bws + B.g[0]);
  half_t* g_next = (half_t*)(bws + B.g[1]);
  // Scale groups, in production order (ids index ChainState: fixed by the architecture, so a replayed graph and a direct run agree).
  // Group 0 is the prologue's g; every BatchNorm backward opens a new group for its dY, and the GEMM results computed from that dY --
  // d a2, d a1, the residual sum g_next -- stay in it (ratio 1).  A downsample branch's dY joins the group of the block's dy0: the
  // two dgrads are summed in place.
  ChainParents par{};
  int n_k = 0;
  auto new_k = [&](int parent) { par.p[n_k] = (unsigned char)parent; return n_k++; };
  int k_g = new_k(0);
  const int total_k = 1 + 3 * A.nblock + 1;
  if (total_k > kChainMax) return neraf_fail(ctx, NERAF_EINVAL, "resnet3d_bwd: chain table too small");
  {
    // d feat is spread over M voxels by the average pool; S0 places the per-voxel gradient's amax at 2^kChainTarget
    const int Mpad = (int)rows_pad(A.final_edge);
    const size_t n = (size_t)Mpad * A.n_features;
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    // the parents of every group, as the loop below assigns them (the prologue runs first: built here from the same rule)
    ChainParents pp{};
    int k = 1, kg = 0;
    for (int b = A.nblock - 1; b >= 0; --b) { pp.p[k] = (unsigned char)kg; pp.p[k + 1] = (unsigned char)k; pp.p[k + 2] = (unsigned char)(k + 1); kg = k + 2; k += 3; }
    pp.p[k] = (unsigned char)kg;                // stem dY
    hipLaunchKernelGGL(bwd_prologue_kernel, dim3(blocks), dim3(256), 0, st, dfeat, scale, kChainTarget + (int)ceilf(log2f((float)Mlast)), Mlast, Mpad,
                       A.n_features, g, reinterpret_cast<ChainState*>(bws + B.chain), reinterpret_cast<unsigned*>(bws + B.amax), total_k, pp);
    neraf_node(ctx, "bwd_prologue_kernel | S0, scale groups, average-pool backward", 0.0, 4096.0 + (double)total_k * kAmaxRep * 4.0, (double)n * 2.0);
  }
  half_t* gm = (half_t*)(bws + B.gm); half_t* da = (half_t*)(bws + B.da);
  WgradItem items[64]; int n_items = 0;     // every weight gradient is computed by ONE grouped launch at the end
  bool g_sums_done = false;                 // the BatchNorm-backward sums of the NEXT block's bn3 were reduced by the dgrad that produced g
  for (int b = A.nblock - 1; b >= 0; --b) {
    const BlockSpec& Bk = A.block[b];
    const int i0 = Bk.conv[0], i1 = Bk.conv[1], i2 = Bk.conv[2];
    const half_t* out = (const half_t*)(ws + L.out[b]);
    const half_t* a1 = (const half_t*)(ws + L.a1[b]);
    const half_t* a2 = (const half_t*)(ws + L.a2[b]);
    const half_t* x_in = b == 0 ? (const half_t*)(ws + L.act_pool) : (const half_t*)(ws + L.out[b - 1]);
    half_t* dy0 = (half_t*)(bws + B.dy[i0]); half_t* dy1 = (half_t*)(bws + B.dy[i1]); half_t* dy2 = (half_t*)(bws + B.dy[i2]);
    half_t* dyds = Bk.ds >= 0 ? (half_t*)(bws + B.dy[Bk.ds]) : nullptr;
    const int k2 = new_k(k_g), k1 = new_k(k2), k0 = new_k(k1);       // groups of dy2 (+ d a2), dy1 (+ d a1), dy0 (+ dyds, g_next)
    // out = relu(bn3(c3) + residual): dy = g * (out > 0) feeds bn3 and the residual branch (the masked copy joins dy0's group, where
    // the identity residual is added)
    if (int e = bn_backward(c, i2, g, nullptr, out, dy2, Bk.ds < 0 ? gm : nullptr, k_g, k2, k0, g_sums_done)) return e;
    g_sums_done = false;
    items[n_items++] = wgrad_item(c, i2, dy2, a2, k2);
    const bool f1 = fuse_bn_sums(A.conv[i1]);                                  // d a2 feeds bn2 (mask a2)
    if (int e = conv_dgrad(c, i2, dy2, nullptr, da, f1 ? i1 : -1, f1 ? a2 : nullptr)) return e;                 // d a2
    if (int e = bn_backward(c, i1, da, nullptr, a2, dy1, nullptr, k2, k1, -1, f1)) return e;
    items[n_items++] = wgrad_item(c, i1, dy1, a1, k1);
    // d a1 feeds bn1 (mask a1); the stride-2 conv2 of a layer's first block runs the parity-class dgrad, which has no statistics epilogue
    const bool f0 = fuse_bn_sums(A.conv[i0]) && A.conv[i1].stride == 1;
    if (int e = conv_dgrad(c, i1, dy1, nullptr, da, f0 ? i0 : -1, f0 ? a1 : nullptr)) return e;                 // d a1
    if (int e = bn_backward(c, i0, da, nullptr, a1, dy0, nullptr, k1, k0, -1, f0)) return e;
    items[n_items++] = wgrad_item(c, i0, dy0, x_in, k0);
    if (Bk.ds >= 0) {
      if (int e = bn_backward(c, Bk.ds, g, nullptr, out, dyds, nullptr, k_g, k0, -1)) return e;
      items[n_items++] = wgrad_item(c, Bk.ds, dyds, x_in, k0);
      // the residual branch's gradient w.r.t. x_in is ADDED IN PLACE: a strided 1x1x1 branch reaches one voxel in eight, and the
      // parity-class dgrad (ConvGeom::tclass) then skips the other seven classes' tiles altogether
      if (int e = conv_dgrad(c, i0, dy0, nullptr, g_next)) return e;
      if (int e = conv_dgrad(c, Bk.ds, dyds, g_next, g_next)) return e;
    } else {
      // identity residual: g_next = dgrad + gm is the gradient w.r.t. the previous block's output out_{b-1} = relu(bn3 + residual):
      // its mask and the sums of that block's bn3 ride on this epilogue -- unless that block has a downsample branch (its second
      // BatchNorm needs its own pair of sums from the same gradient: both keep their launches)
      const bool fg = b > 0 && A.block[b - 1].ds < 0 && fuse_bn_sums(A.conv[A.block[b - 1].conv[2]]);
      if (int e = conv_dgrad(c, i0, dy0, gm, g_next, fg ? A.block[b - 1].conv[2] : -1, fg ? (const half_t*)(ws + L.out[b - 1]) : nullptr)) return e;
      g_sums_done = fg;
    }
    half_t* t = g; g = g_next; g_next = t;
    k_g = k0;
  }
  // stem: max-pool -> relu -> bn1 -> conv1
  {
    const ConvSpec& c0 = A.conv[0];
    half_t* dpost = (half_t*)(bws + B.dpost);          // the fp32-sized buffer, used as fp16
    const size_t rp = rows_pad(c0.dout);
    hipLaunchKernelGGL(maxpool_bwd_gather_kernel, dim3(gather_blocks(c0.dout)), dim3(256), 0, st,
                       (const unsigned char*)(ws + L.pool_arg), c0.dout, A.pooled, g, dpost, rp);
    NERAF_HIP_CHECK(ctx, hipGetLastError());
    neraf_node(ctx, "maxpool_bwd_gather_kernel | max-pool routing", 0.0, (double)cube(A.pooled) * 64 * 3.0, (double)rp * 64 * 2.0);
    half_t* dy0 = (half_t*)(bws + B.dy[0]);
    const int k_s = new_k(k_g);
    if (int e = bn_backward(c, 0, dpost, nullptr, nullptr, dy0, nullptr, k_g, k_s, -1)) return e;      // relu mask already applied by the routing
    items[n_items++] = wgrad_item(c, 0, dy0, (const half_t*)(ws + L.x0), k_s);
    if (n_cells > 0) {
      if (!stem_wt_packed(A)) return neraf_fail(ctx, NERAF_EINVAL, "resnet3d_bwd: the grid gradient needs the 7 -> 64 channel 5x5x5 stem");
      // Wt[tap][c][co]: written by neraf_resnet3d_pack_weights_bwd into the stem's slot of the packed blob
      const float* Wt = (const float*)((const char*)packed_t + B.wt[0]);
      hipLaunchKernelGGL(stem_dgrid_kernel, dim3((n_cells + 3) / 4), dim3(256), 0, st, dy0, Wt, A.S, c0.dout,
                         reinterpret_cast<const unsigned long long*>(bws + B.scale + 64), n_cells, n_ch, c.inv(k_s), dgrid_cells);
      NERAF_HIP_CHECK(ctx, hipGetLastError());
      // per cell: 27 dY rows of 128 bytes and 27 x 7 weight rows of 256 bytes requested (the table itself is 224 KB, L2-resident)
      neraf_node(ctx, "stem_dgrid_kernel | grid gradient of the refresh window", 2.0 * n_cells * (125.0 / 8.0) * 64 * n_ch,
                 (double)n_cells * 27.0 * 128.0 + 125.0 * 7 * 64 * 4,
                 (double)n_cells * n_ch * 4.0);
    }
  }
  if (n_k != total_k) return neraf_fail(ctx, NERAF_EINVAL, "resnet3d_bwd: scale group count mismatch");
  (void)par;
  // all 43 weight gradients: one TN GEMM grid over every (convolution, tile, K-split) + one reducer
  return launch_wgrad_grouped(ctx, items, n_items, (const half_t*)(ws + L.zero_page), (float*)(bws + B.splitk), B.splitk_bytes, c.inv_base(), st);
}

// Workspaces whose chain exponents have been calibrated (see the header).  neraf_resnet3d_bwd_reset forgets one.
static std::mutex g_calib_mu;
static std::unordered_map<const void*, unsigned> g_calibrated;      // workspace -> passes run since its calibration
constexpr int kMaxCalibrationPasses = 48;

// stage test: a valid ChainState with S0 = 1 and the given exponents for groups 0, 1, 2
__global__ void chain_set_kernel(ChainState* cs, int e0, int e1, int e2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int e[3] = {e0, e1, e2};
  for (int t = 0; t < 3; ++t) { cs->e[t] = e[t]; cs->pow2[t] = exp2f((float)e[t]); cs->inv[t] = exp2f((float)-e[t]); }
  cs->magic = kChainMagic;
}

extern "C" int neraf_resnet3d_bwd_reset(neraf_ctx* ctx, void* bwd_workspace) {
  (void)ctx;
  std::lock_guard<std::mutex> lk(g_calib_mu);
  g_calibrated.erase(bwd_workspace);
  return NERAF_OK;
}

extern "C" int neraf_resnet3d_bwd(neraf_ctx* ctx, const neraf_resnet3d_desc* d, const void* packed_t, const float* const* conv_w,
                                  const float* const* bn, void* workspace, void* bwd_workspace, const float* dfeat,
                                  float* const* w_grads, float* const* bn_grads, size_t cell_start, int n_cells, int n_ch,
                                  float* dgrid_cells, neraf_stream_t stream) {
  Arch A; Layout L; BwdLayout B;
  if (make_arch(d, &A) || !packed_t || !conv_w || !bn || !workspace || !bwd_workspace || !dfeat || !w_grads || !bn_grads ||
      (n_cells > 0 && (!dgrid_cells || n_ch < 1 || n_ch > 7 || cell_start + (size_t)n_cells > cube(d->grid_size))))
    return neraf_fail(ctx, NERAF_EINVAL, "resnet3d_bwd: bad arguments");
  make_layout(A, &L);
  make_bwd_layout(A, &B);
  hipStream_t st = (hipStream_t)stream;
  char* bws = (char*)bwd_workspace;
  // the refresh window moves every step: its start travels through device memory, outside the captured sequence
  hipLaunchKernelGGL(set_u64_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(bws + B.scale + 64),
                     (unsigned long long)cell_start);
  // Producers record their amax on every kTrackPeriod-th pass only (two captured variants of the sequence): the atomics cost ~0.3 us
  // at the tail of each of ~130 launches (+0.06 ms per step when every pass records, profiles/r05_fp16_chain_ab.txt), the magnitudes
  // drift by far less than the 8x headroom in a handful of steps, and an overflow costs a skipped step, not a wrong one.
  // NERAF_CHAIN_AMAX=0: never (frozen scales, measurement only); NERAF_CHAIN_AMAX_PERIOD=n: every n-th pass.
  static const bool track_env = [] { const char* e = getenv("NERAF_CHAIN_AMAX"); return !(e && atoi(e) == 0); }();
  static const unsigned period = [] { const char* e = getenv("NERAF_CHAIN_AMAX_PERIOD"); const int v = e ? atoi(e) : 4; return (unsigned)(v < 1 ? 1 : v); }();
  auto run = [&](hipStream_t s2, bool track) {
    return resnet3d_bwd_body(ctx, A, L, B, packed_t, conv_w, bn, (char*)workspace, bws, dfeat, w_grads, bn_grads, n_cells, n_ch, dgrid_cells, s2,
                             track);
  };

  // First use of this workspace: the chain's exponents start at 0 relative to S0 (the ChainState is marked invalid) and are calibrated
  // by running the chain on this very gradient until a prologue reports that every tensor of the pass before it was stored as finite
  // fp16 from finite inputs (ChainState::unsettled; one device-to-host read per pass -- this happens once per workspace).  The
  // results of the calibration passes are overwritten by the real pass below.
  bool fresh;
  unsigned pass_no;
  {
    std::lock_guard<std::mutex> lk(g_calib_mu);
    auto it = g_calibrated.find(bwd_workspace);
    fresh = it == g_calibrated.end();
    if (fresh) it = g_calibrated.emplace(bwd_workspace, 0u).first;
    pass_no = it->second++;
  }
  const bool track = track_env && (pass_no % period) == 0;
  auto body = [&](hipStream_t s2) { return run(s2, track); };
  if (fresh) {
    // calibration passes are set-up work: they stay out of the per-kernel event statistics (neraf_prof_enable)
    struct ProfPause { neraf_ctx* c; bool was; ProfPause(neraf_ctx* c_) : c(c_), was(c_ && c_->prof) { if (c) c->prof = false; }
                       ~ProfPause() { if (c) c->prof = was; } } pause(ctx);
    auto forget = [&] { std::lock_guard<std::mutex> lk(g_calib_mu); g_calibrated.erase(bwd_workspace); };
    NERAF_HIP_CHECK(ctx, hipMemsetAsync(bws + B.chain, 0, sizeof(ChainState), st));
    bool settled = false, postponed = false;
    unsigned unsettled = 0;
    for (int i = 0; i < kMaxCalibrationPasses && !settled && !postponed; ++i) {
      if (int e = run(st, true)) { forget(); return e; }
      struct { unsigned unsettled, passes, dfeat_bad; } rd = {0u, 0u, 0u};
      static_assert(offsetof(ChainState, dfeat_bad) == offsetof(ChainState, unsettled) + 8, "read as one block");
      hipError_t he = hipMemcpyAsync(&rd, bws + B.chain + offsetof(ChainState, unsettled), sizeof(rd), hipMemcpyDeviceToHost, st);
      if (he == hipSuccess) he = hipStreamSynchronize(st);
      if (he != hipSuccess) { forget(); NERAF_HIP_CHECK(ctx, he); }
      unsettled = rd.unsettled;
      // an overflowed d feat (the GradScaler's first steps) has no magnitude to calibrate on: this step's gradients are inf whatever
      // the exponents, the optimizer will skip it, and the next backward calibrates
      postponed = rd.dfeat_bad != 0;
      settled = i >= 1 && unsettled == 0;         // the pass before this one was clean, and this one ran on exponents re-centred from it
    }
    if (postponed) forget();
    else if (!settled) {
      // never silently: the real pass would run on uncalibrated exponents and every later step would carry inf gradients
      forget();
      char msg[200];
      snprintf(msg, sizeof(msg), "resnet3d_bwd: the fp16 gradient chain did not calibrate in %d passes (%u scale groups still overflow): "
               "non-finite activations or weights?", kMaxCalibrationPasses, unsettled);
      return neraf_fail(ctx, NERAF_ESTATE, msg);
    }
  }
  ArgHash k;
  k.add(0x62776432u); k.add(d->grid_size); k.add(packed_t); k.ptrs((const void* const*)conv_w, A.nconv);
  k.ptrs((const void* const*)bn, 4 * A.nconv); k.add(workspace); k.add(bwd_workspace); k.add(dfeat);
  k.ptrs((const void* const*)w_grads, A.nconv); k.ptrs((const void* const*)bn_grads, 2 * A.nconv);
  k.add(n_cells); k.add(n_ch); k.add(dgrid_cells); k.add(track);
  return neraf_run_graphed(ctx, st, k.h, body);
}

// Test aid: the chain's state after the last pass -- exponents e[t] and the amax each tensor's producer recorded in that pass (as
// floats; the next prologue consumes and clears them).  n = number of entries the caller's arrays hold.
extern "C" int neraf_resnet3d_bwd_chain_state(neraf_ctx* ctx, const neraf_resnet3d_desc* d, const void* bwd_workspace, int32_t* e_out,
                                              float* amax_out, int n, int32_t* info2, neraf_stream_t stream) {
  Arch A; BwdLayout B;
  if (make_arch(d, &A) || !bwd_workspace || !e_out || !amax_out || n < 1 || n > kChainMax)
    return neraf_fail(ctx, NERAF_EINVAL, "resnet3d_bwd_chain_state: bad arguments");
  make_bwd_layout(A, &B);
  const char* bws = (const char*)bwd_workspace;
  NERAF_HIP_CHECK(ctx, hipStreamSynchronize((hipStream_t)stream));
  ChainState cs;
  NERAF_HIP_CHECK(ctx, hipMemcpy(&cs, bws + B.chain, sizeof(cs), hipMemcpyDeviceToHost));
  std::vector<unsigned> am((size_t)n * kAmaxRep * kAmaxStride);
  NERAF_HIP_CHECK(ctx, hipMemcpy(am.data(), bws + B.amax, am.size() * 4, hipMemcpyDeviceToHost));
  for (int t = 0; t < n; ++t) {
    unsigned mx = 0;
    for (int r = 0; r < kAmaxRep; ++r) mx = std::max(mx, am[((size_t)t * kAmaxRep + r) * kAmaxStride]);
    float f; memcpy(&f, &mx, 4);
    e_out[t] = cs.magic == kChainMagic ? cs.e[t] : 0;
    amax_out[t] = f;
  }
  if (info2) { info2[0] = (int32_t)cs.unsettled; info2[1] = (int32_t)cs.passes; }
  return NERAF_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Test entry: the max-pool routing of the backward alone.  arg uint8 [dout^3][64] (the forward's table), g fp16 [dout^3][64],
// dout = (din - 1) / 2 + 1; writes dpost fp16 [round_up(din^3, 128)][64].
extern "C" int neraf_debug_maxpool_bwd(neraf_ctx* ctx, const void* arg, const void* g, int din, void* dpost, neraf_stream_t stream) {
  if (!arg || !g || !dpost || din < 2 || din > 256) return neraf_fail(ctx, NERAF_EINVAL, "debug_maxpool_bwd: bad arguments");
  hipLaunchKernelGGL(maxpool_bwd_gather_kernel, dim3(gather_blocks(din)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)arg,
                     din, (din - 1) / 2 + 1, (const half_t*)g, (half_t*)dpost, rows_pad(din));
  NERAF_HIP_CHECK(ctx, hipGetLastError());
  return NERAF_OK;
}

// Test entry: ONE conv + BatchNorm(train) + ReLU stage, forward statistics and backward, on caller data.  The full
// encoder is chaotic under fp16 rounding through its ReLU gates, so besides the gate-matched full-chain test
// (tests/test_gpu_resnet3d.py::test_resnet3d_backward_gate_matched) the backward kernels are verified stage by stage against
// autograd here (::test_conv_bn_relu_stage_backward).
//   x    fp16 [din^3][cin]          w fp32 [cout][cin_real][k^3]        gamma, beta fp32 [cout]
//   g    fp32 [dout^3][cout]  upstream gradient w.r.t. relu(bn(conv(x)))
//   out: y fp16 [dout^3][cout] (post ReLU), dx fp32 [din^3][cin] (skipped for the stem), dw fp32 like w, dgamma, dbeta
extern "C" int neraf_debug_conv_bn_relu_stage(neraf_ctx* ctx, int cin, int cin_real, int cout, int k, int stride, int pad, int din,
                                              const void* x_f16, const float* w, const float* gamma, const float* beta, const float* g,
                                              void* y_f16, float* dx, float* dw, float* dgamma, float* dbeta, neraf_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  Arch A{};
  A.S = din; A.nconv = 1; A.nblock = 0; A.pooled = din; A.final_edge = din; A.n_features = 1024;
  const int dout = (din + 2 * pad - k) / stride + 1;
  A.conv[0] = ConvSpec{cin, cout, k, stride, pad, din, dout, cin_real};
  Layout L{}; BwdLayout B{};
  make_layout(A, &L);
  make_bwd_layout(A, &B);
  // the stem branch of make_bwd_layout skips conv 0 when sizing activation buffers: size them for this stage explicitly
  const size_t act = std::max(rows_pad(dout) * (size_t)cout, rows_pad(din) * (size_t)cin) * 2 + 256;
  char *ws = nullptr, *bws = nullptr, *packed = nullptr, *packed_t = nullptr, *extra = nullptr;
  NERAF_HIP_CHECK(ctx, hipMalloc(&ws, L.total));
  NERAF_HIP_CHECK(ctx, hipMalloc(&bws, B.total));
  NERAF_HIP_CHECK(ctx, hipMalloc(&packed, L.packed_total));
  NERAF_HIP_CHECK(ctx, hipMalloc(&packed_t, B.packed_total + 256));
  NERAF_HIP_CHECK(ctx, hipMalloc(&extra, 5 * act));
  NERAF_HIP_CHECK(ctx, hipMemsetAsync(ws, 0, L.total, st));
  NERAF_HIP_CHECK(ctx, hipMemsetAsync(bws, 0, B.total, st));
  NERAF_HIP_CHECK(ctx, hipMemsetAsync(extra, 0, 5 * act, st));
  const float* wl[1] = {w};
  // forward: pack, conv (+stats), bn+relu
  {
    PackTable t{};
    t.n = 1; t.src[0] = w; t.begin[0] = 0; t.dst_off[0] = L.w[0]; t.cout[0] = cout; t.cin_real[0] = cin_real; t.cin[0] = cin;
    t.taps[0] = k * k * k; t.kpad[0] = conv_kpad(A.conv[0]); t.begin[1] = (unsigned long long)conv_npad(A.conv[0]) * conv_kpad(A.conv[0]);
    hipLaunchKernelGGL(pack_all_conv_weights_kernel, dim3((unsigned)((t.begin[1] + 255) / 256)), dim3(256), 0, st, t, packed);
  }
  half_t* xin = (half_t*)extra;                      // padded copy of the input
  NERAF_HIP_CHECK(ctx, hipMemcpyAsync(xin, x_f16, cube(din) * cin * 2, hipMemcpyDeviceToDevice, st));
  if (int e = run_conv(ctx, st, A, L, 0, packed, ws, xin)) return e;
  const float* bnp[4] = {gamma, beta, gamma, gamma};
  half_t* yact = (half_t*)(extra + act);
  {
    BnApplyArgs a{};
    a.a = bn_src_fwd(A, L, ws, bnp, 0, 1);
    a.M = (int)cube(dout); a.Mpad = (int)rows_pad(dout); a.C = cout; a.relu = 1; a.out = yact;
    if (int e = run_bn_apply(ctx, st, a)) return e;
  }
  NERAF_HIP_CHECK(ctx, hipMemcpyAsync(y_f16, yact, cube(dout) * cout * 2, hipMemcpyDeviceToDevice, st));
  // backward
  if (dx && cin % 64 == 0) {
    PackTTable t{};
    const int nrows = cin == 64 || cin == 8 ? 64 : round_up(cin, 128);
    t.n = 1; t.src[0] = w; t.tile_begin[0] = 0; t.dst_off[0] = B.wt[0]; t.cout[0] = cout; t.cin[0] = cin_real; t.taps[0] = k * k * k;
    t.kcols[0] = t.taps[0] * cout; t.nrows[0] = nrows;
    t.tile_begin[1] = (cout / 32) * (nrows / 32);
    if (int e = launch_pack_dgrad(ctx, t, t.tile_begin[1], t.taps[0], packed_t, st)) return e;
  }
  float* wg[1] = {dw};
  float* bng[2] = {dgamma, dbeta};
  Ctx c{ctx, st, &A, &L, &B, packed_t, ws, bws, bnp, wg, bng};
  // scale groups of the stage: 0 = g (fp32, unscaled), 1 = dy and its dgrad result (stored x 2^6): the re-scaling path is exercised
  hipLaunchKernelGGL(chain_set_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<ChainState*>(bws + B.chain), 0, 6, 0);
  half_t* dy = (half_t*)(extra + 2 * act);
  half_t* dxb = (half_t*)(extra + 3 * act);
  if (int e = bn_backward(c, 0, nullptr, g, yact, dy, nullptr, 0, 1, -1)) return e;
  if (int e = conv_wgrad(c, 0, dy, xin, 1)) return e;
  if (dx && cin % 64 == 0) {
    if (int e = conv_dgrad(c, 0, dy, nullptr, dxb)) return e;
    const size_t n = cube(din) * cin;
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dxb, n, c.inv(1), dx);
  }
  NERAF_HIP_CHECK(ctx, hipStreamSynchronize(st));
  (void)wl;
  (void)hipFree(ws); (void)hipFree(bws); (void)hipFree(packed); (void)hipFree(packed_t); (void)hipFree(extra);
  return NERAF_OK;
}

// Test entry: the raw stem convolution (7 -> 64 channels, 5x5x5, stride 2, pad 2: conv loader 2) on caller data, straight into the
// caller's buffers.  x fp16 [din^3][8] (only the first cin_real channels carry weights), w fp32 [64][cin_real][125];
// y fp16 [din^3 / 8 rounded up to 128 rows][64] (rows past the result are written as zeros), sums fp32 [2][128] = column sums and
// sums of squares of the result (the fused BatchNorm statistics, one replica, cleared here).
extern "C" int neraf_debug_stem_conv(neraf_ctx* ctx, int din, int cin_real, const void* x_f16, const float* w, void* y_f16, float* sums,
                                     neraf_stream_t stream) {
  if (!x_f16 || !w || !y_f16 || !sums || din < 2 || din > 256 || (din & 1) || cin_real < 1 || cin_real > 8)
    return neraf_fail(ctx, NERAF_EINVAL, "debug_stem_conv: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const ConvSpec c{8, 64, 5, 2, 2, din, din / 2, cin_real};
  const size_t wbytes = (size_t)conv_npad(c) * conv_kpad(c) * 2;
  char *packed = nullptr, *zero = nullptr;
  NERAF_HIP_CHECK(ctx, hipMalloc(&packed, wbytes));
  NERAF_HIP_CHECK(ctx, hipMalloc(&zero, 256));
  NERAF_HIP_CHECK(ctx, hipMemsetAsync(zero, 0, 256, st));
  NERAF_HIP_CHECK(ctx, hipMemsetAsync(sums, 0, 256 * 4, st));
  PackTable t{};
  t.n = 1; t.src[0] = w; t.begin[0] = 0; t.dst_off[0] = 0; t.cout[0] = 64; t.cin_real[0] = cin_real; t.cin[0] = 8;
  t.taps[0] = 125; t.kpad[0] = conv_kpad(c); t.begin[1] = (unsigned long long)conv_npad(c) * conv_kpad(c);
  hipLaunchKernelGGL(pack_all_conv_weights_kernel, dim3((unsigned)((t.begin[1] + 255) / 256)), dim3(256), 0, st, t, packed);
  GemmParams g{};
  g.A = (const half_t*)x_f16; g.lda = 8;
  g.B = (const half_t*)packed; g.ldb = conv_kpad(c);
  g.M = (int)cube(c.dout); g.N = 64; g.K = conv_kpad(c); g.Mpad = (int)rows_pad(c.dout); g.Npad = 64; g.alpha = 1.f; g.tile_n = 64;
  g.C16 = (half_t*)y_f16; g.ldc16 = 64;
  g.colsum = sums; g.colsumsq = sums + 128;
  g.conv.loader = 2; g.conv.din = din; g.conv.dout = c.dout; g.conv.stride = 2; g.conv.pad = 2; g.conv.ksize = 5; g.conv.cin = 8;
  g.conv.zero_page = (const half_t*)zero;
  const int e = launch_gemm_f16(ctx, g, st);
  NERAF_HIP_CHECK(ctx, hipStreamSynchronize(st));
  (void)hipFree(packed); (void)hipFree(zero);
  return e;
}

// Test entry: a raw stride-2 transposed convolution (the dgrad GEMM of a k^3, stride-2, pad k/2 convolution cin -> cout whose input
// edge is din) on caller data.  dy fp16 [(din/2)^3][cout], w fp32 [cout][cin][k^3]; dx fp16 [din^3][cin] (din^3 a multiple of 128):
// in_place != 0 adds the result into dx (add16 == destination: what the residual branch's dgrad does), else dx is overwritten.
extern "C" int neraf_debug_conv_transpose(neraf_ctx* ctx, int cin, int cout, int k, int din, const void* dy_f16, const float* w,
                                          void* dx_f16, int in_place, neraf_stream_t stream) {
  if (!dy_f16 || !w || !dx_f16 || (k != 1 && k != 3) || din < 2 || din > 64 || (din & 1) || (cube(din) % 128) || cin < 64 || (cin % 64) ||
      cout < 64 || (cout % 64))
    return neraf_fail(ctx, NERAF_EINVAL, "debug_conv_transpose: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  Arch A{};
  A.S = din; A.nconv = 1; A.nblock = 0; A.pooled = din; A.final_edge = din; A.n_features = 1024;
  A.conv[0] = ConvSpec{cin, cout, k, 2, k / 2, din, din / 2, cin};
  Layout L{}; BwdLayout B{};
  make_layout(A, &L);
  make_bwd_layout(A, &B);
  char *ws = nullptr, *bws = nullptr, *packed_t = nullptr;
  NERAF_HIP_CHECK(ctx, hipMalloc(&ws, L.total));
  NERAF_HIP_CHECK(ctx, hipMalloc(&bws, B.total));
  NERAF_HIP_CHECK(ctx, hipMalloc(&packed_t, B.packed_total + 256));
  NERAF_HIP_CHECK(ctx, hipMemsetAsync(ws + L.zero_page, 0, 256, st));
  PackTTable t{};
  const int nrows = cin == 64 ? 64 : round_up(cin, 128);
  t.n = 1; t.src[0] = w; t.tile_begin[0] = 0; t.dst_off[0] = B.wt[0]; t.cout[0] = cout; t.cin[0] = cin; t.taps[0] = k * k * k;
  t.kcols[0] = t.taps[0] * cout; t.nrows[0] = nrows;
  t.tile_begin[1] = (cout / 32) * (nrows / 32);
  int e = launch_pack_dgrad(ctx, t, t.tile_begin[1], t.taps[0], packed_t, st);
  if (!e) {
    Ctx c{ctx, st, &A, &L, &B, packed_t, ws, bws, nullptr, nullptr, nullptr};
    e = conv_dgrad(c, 0, (const half_t*)dy_f16, in_place ? (const half_t*)dx_f16 : nullptr, (half_t*)dx_f16);
  }
  NERAF_HIP_CHECK(ctx, hipStreamSynchronize(st));
  (void)hipFree(ws); (void)hipFree(bws); (void)hipFree(packed_t);
  return e;
}

// Test entry: the stem's grid gradient (stem_dgrid_kernel) for the window of n_cells cells from cell `start` of the S^3 grid (cell =
// (z S + y) S + x), on caller data: dy fp16 [(S/2)^3][64] (gradient w.r.t. the stem convolution's output), w fp32 [64][7][125];
// out fp32 [n_ch][n_cells] = inv_scale * the transposed convolution at those cells, channels 0 .. n_ch - 1.
extern "C" int neraf_debug_stem_dgrid(neraf_ctx* ctx, int S, const void* dy_f16, const float* w, unsigned long long start, int n_cells,
                                      int n_ch, float inv_scale, float* out, neraf_stream_t stream) {
  if (!dy_f16 || !w || !out || S < 2 || S > 256 || (S & 1) || n_cells < 1 || n_ch < 1 || n_ch > 7 || start + (size_t)n_cells > cube(S))
    return neraf_fail(ctx, NERAF_EINVAL, "debug_stem_dgrid: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  char* tmp = nullptr;                         // [0, 8): start, [64, 72): inv_scale, [256, ...): Wt
  NERAF_HIP_CHECK(ctx, hipMalloc(&tmp, 256 + (size_t)kStemWtElems * 4));
  hipLaunchKernelGGL(set_u64_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<unsigned long long*>(tmp), start);
  hipLaunchKernelGGL(set_f32x2_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<float*>(tmp + 64), inv_scale, 0.f);
  hipLaunchKernelGGL(stem_w_relayout_kernel, dim3((kStemWtElems + 255) / 256), dim3(256), 0, st, w, reinterpret_cast<float*>(tmp + 256));
  hipLaunchKernelGGL(stem_dgrid_kernel, dim3((n_cells + 3) / 4), dim3(256), 0, st, (const half_t*)dy_f16, reinterpret_cast<const float*>(tmp + 256),
                     S, S / 2, reinterpret_cast<const unsigned long long*>(tmp), n_cells, n_ch, reinterpret_cast<const float*>(tmp + 64), out);
  NERAF_HIP_CHECK(ctx, hipGetLastError());
  NERAF_HIP_CHECK(ctx, hipStreamSynchronize(st));
  (void)hipFree(tmp);
  return NERAF_OK;
}
