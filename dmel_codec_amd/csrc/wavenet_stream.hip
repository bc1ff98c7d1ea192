// One-launch STREAMING step for narrow, unconditioned WaveNets (the dMel ENCODER fed from a microphone: 10 -> 70 channels, 20 gated
// dilated blocks, ~30 new frames per push): dmel_wavenet_stream_step_ex on the new columns of every level in ONE launch.
//
// The layered step is ~45 dependent launches of 8-128 workgroups per push (input projection, 20 x (gate conv, copy, res/skip conv),
// skip projection): launch- and latency-bound, the regime wavenet_fused.hip was written to escape.  Here, in the image of
// wavenet_fused_kernel, one workgroup owns one (utterance, group) item for all blocks of the push:
//   * for block l the window [prev[l+1] - 8, prev[l+1] + 96 + 8) of level l is staged from the history buffer into LDS -- an fp32 master
//     copy of the <= 96 new columns (the residual update must stay exact) and the exact three-way bf16 split of the whole window in
//     B-fragment order [piece][8-channel group][column + 8 halo][8]; a tap is a column offset.  Columns before absolute frame 0 and
//     columns at or behind the level's frontier read as ZERO: the host only lets a window reach past the frontier when the frontier is
//     the end of the sequence (the final step), so an interior edge always reads history;
//   * the same fifteen waves, the same six partial products per 32 x 32 x 16 block in the same order, K walked chunk-major / tap-minor,
//     the same epilogue expressions as wavenet_fused_kernel and the layered kernels: IDENTICAL bits;
//   * the new columns of level l + 1 go to the history, and the skip contribution is added into the absolute-time skip buffer IN LAYER
//     ORDER -- the frontiers are staggered by the dilations, so a column's skip sum is completed over several pushes and cannot live in
//     registers as it does in the whole-sequence kernel;
//   * the next block reads its window back from the history (L2): a workgroup's own stores are visible to it after the barrier;
//   * input projection (+ SiLU) in front on the new columns of level 0, skip_projection behind on the columns whose sum is complete,
//     output mask in the store.
// Eligibility = that of the whole-sequence kernel (residual channels <= 80, no condition, no output projection, dilations <= 8) and at
// most 96 new columns per level per launch; a larger push is cut into consecutive sub-steps by the host code below.
//
// Nothing above needs the items of a launch to agree on their frontiers: a workgroup only ever touches its own item.  The per-item form
// (dmel_wavenet_stream_step_items: independent live sessions in one launch) is the same kernel body reading prev / next / the block count
// from its utterance's row of a device table instead of the launch arguments; a row that has nothing to do leaves before the first barrier.
#include "ops.h"

namespace dmel {

typedef float fx16 __attribute__((ext_vector_type(16)));
typedef __bf16 fbf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int kST = 96;                 // new columns per level and launch (three 32-column MFMA blocks)
constexpr int kSH = 8;                  // halo columns on each side (max dilation)
constexpr int kSXS = kST + 2 * kSH;     // staged row length of a window
constexpr int kSPD = 3;                 // weight prefetch distance in K steps (kSPD + 1 register sets)

struct StreamArgs {
  const float* x;            // (N, Cin, cap) raw input, nullable (no input projection: the caller writes level 0)
  float* hist;               // (L + 1, N, C, cap)
  float* skip;               // (N, C, cap)
  float* y;                  // (N, C, cap)
  const int64_t* out_len;    // nullable, (N / len_div), relative to column 0
  int len_div, N, Cin, C, L, cycle, has_in, nblk;   // nblk: blocks 0 .. nblk - 1 have new columns
  int64_t cap;
  float skip_scale;
  const void* in_w;
  const float* in_b;
  const void* skip_w;
  const float* skip_b;
  const void* const* gate_w;
  const float* const* gate_b;
  const void* const* rs_w;
  const float* const* rs_b;
  int prev[kStreamMaxL + 1], next[kStreamMaxL + 1];
  // per-item form (dmel_wavenet_stream_step_items): row n / len_div of `tab` replaces prev / next / nblk for workgroup n
  const int32_t* tab;        // (N / len_div, kStreamRowInts(L)): prev[0..L] | next[0..L] | block count, < 0 = idle row
};

__device__ __forceinline__ uint32_t s_pack_hi16(float lo, float hi) {
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
// exact three-way split of four consecutive channels -> one 8-byte LDS store per piece (as wavenet_fused.hip)
__device__ __forceinline__ void s_split4_store(const float (&v)[4], char* p0, char* p1, char* p2) {
  float r[4], s[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[e] = v[e] - __uint_as_float(__float_as_uint(v[e]) & 0xffff0000u);
    s[e] = r[e] - __uint_as_float(__float_as_uint(r[e]) & 0xffff0000u);
  }
  *reinterpret_cast<uint2*>(p0) = make_uint2(s_pack_hi16(v[0], v[1]), s_pack_hi16(v[2], v[3]));
  *reinterpret_cast<uint2*>(p1) = make_uint2(s_pack_hi16(r[0], r[1]), s_pack_hi16(r[2], r[3]));
  *reinterpret_cast<uint2*>(p2) = make_uint2(s_pack_hi16(s[0], s[1]), s_pack_hi16(s[2], s[3]));
}
// eight consecutive channels of one column -> one 16-byte unit per piece
__device__ __forceinline__ void s_split8_store(const float (&v)[8], uint4* d0, uint4* d1, uint4* d2) {
  uint32_t p1[4], p2[4], p3[4];
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const float r0 = v[e] - __uint_as_float(__float_as_uint(v[e]) & 0xffff0000u);
    const float r1 = v[e + 1] - __uint_as_float(__float_as_uint(v[e + 1]) & 0xffff0000u);
    const float s0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u);
    const float s1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
    p1[e >> 1] = s_pack_hi16(v[e], v[e + 1]);
    p2[e >> 1] = s_pack_hi16(r0, r1);
    p3[e >> 1] = s_pack_hi16(s0, s1);
  }
  *d0 = make_uint4(p1[0], p1[1], p1[2], p1[3]);
  *d1 = make_uint4(p2[0], p2[1], p2[2], p2[3]);
  *d2 = make_uint4(p3[0], p3[1], p3[2], p3[3]);
}

// NCH = 16-channel chunks of the residual width (C <= 16 NCH); NG = 2 NCH eight-channel groups.
// ITEMS: the frontiers are this workgroup's row of a.tab instead of the launch's a.prev / a.next / a.nblk.  Every thread reads the row at
// the same addresses and nothing writes the table while the kernel runs, so whatever is derived from it -- the idle early-out, the
// block count, every trip count around a barrier -- is uniform across the workgroup; readfirstlane keeps the values in scalar registers.
template <int NCH, bool ITEMS>
__global__ __launch_bounds__(192 * NCH) void wavenet_stream_kernel(StreamArgs a) {
  constexpr int NG = 2 * NCH, CP = 16 * NCH, NW = 3 * NCH, NTHR = 64 * NW;
  constexpr int GS = 3 * NCH, RS = NCH, LS = GS + RS;             // K steps of the gated conv, of the projection, per block
  static_assert(LS % (kSPD + 1) == 0, "the weight register sets must rotate consistently across blocks");
  extern __shared__ __attribute__((aligned(16))) char lds_stream[];
  uint4* Xp = reinterpret_cast<uint4*>(lds_stream);               // [3][NG][kSXS]   window of the block's input level, split, with halo
  uint4* Zp = Xp + 3 * NG * kSXS;                                 // [3][NG][kST]    gate output z / projection inputs, split
  float* Xf = reinterpret_cast<float*>(Zp + 3 * NG * kST);        // [CP][kST]       the new columns of the input level, fp32 master
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const int wave = wv / 3, nb = wv - 3 * wave;          // row tile, column block of this wave
  const int q = nb * 32 + l31;                          // this lane's column of the launch's new columns
  const int n = blockIdx.x, C = a.C;
  const int32_t* row = ITEMS ? a.tab + (size_t)(n / a.len_div) * kStreamRowInts(a.L) : nullptr;
  auto PREV = [&](int l) -> int {
    if constexpr (ITEMS) return __builtin_amdgcn_readfirstlane(row[l]);
    else return a.prev[l];
  };
  auto NEXT = [&](int l) -> int {
    if constexpr (ITEMS) return __builtin_amdgcn_readfirstlane(row[a.L + 1 + l]);
    else return a.next[l];
  };
  int nblk = a.nblk;
  if constexpr (ITEMS) {
    nblk = __builtin_amdgcn_readfirstlane(row[2 * (a.L + 1)]);
    if (nblk < 0) return;                               // idle item: before the first barrier, nothing is written
  }
  const int64_t cap = a.cap;
  const int64_t item = (int64_t)n * C * cap, lvl = (int64_t)a.N * C * cap;
  const int olim = a.out_len ? (int)min(a.out_len[n / a.len_div], (int64_t)0x7fffffff) : 0x7fffffff;
  const uint32_t lane16 = lane * 16;

  // ---- zero the split buffers once: channel padding must read as zeros forever
  for (int i = tid; i < 3 * NG * (kSXS + kST); i += NTHR) Xp[i] = make_uint4(0, 0, 0, 0);
  for (int i = tid; i < CP * kST; i += NTHR) Xf[i] = 0.f;
  __syncthreads();

  fx16 acc;
  auto zero_acc = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  };
  auto mma_step = [&](const uint4 (&w)[3], const uint4* src, int row_len, int c16, int col0) {
    const uint4* bp = src + (2 * c16 + h) * row_len + col0 + q;
    fbf16x8 b[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) b[p] = __builtin_bit_cast(fbf16x8, bp[p * NG * row_len]);
    constexpr int PA[6] = {2, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};   // smallest partial products first (as conv_bf16_kernel)
#pragma unroll
    for (int t = 0; t < 6; ++t)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(fbf16x8, w[PA[t]]), b[PB[t]], acc, 0, 0, 0);
  };
  auto load_w = [&](uint4 (&dst)[3], const void* image, int steps, int step) {
    const char* sp = reinterpret_cast<const char*>(image) + ((size_t)wave * steps + step) * 3072 + lane16;
#pragma unroll
    for (int p = 0; p < 3; ++p) dst[p] = *reinterpret_cast<const uint4*>(sp + p * 1024);
  };
  auto slot = [&](uint4* buf, int row_len, int p, int c0, int j) -> char* {
    return reinterpret_cast<char*>(buf + (p * NG + (c0 >> 3)) * row_len + j) + (c0 & 7) * 2;
  };

  // ---- level 0: silu(input_projection(x)) on its new columns [prev[0], next[0])       (wavenet.py:205-207)
  if (a.has_in && NEXT(0) > PREV(0)) {
    const int p0 = PREV(0), W0 = NEXT(0) - p0;
    const float* xin = a.x + (int64_t)n * a.Cin * cap + p0;
    for (int i = tid; i < 2 * kST; i += NTHR) {          // raw input (<= 16 channels: one chunk) into Zp groups 0..1
      const int g = i / kST, qq = i - g * kST;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        v[e] = (c < a.Cin && qq < W0) ? xin[(int64_t)c * cap + qq] : 0.f;
      }
      s_split8_store(v, Zp + (0 * NG + g) * kST + qq, Zp + (1 * NG + g) * kST + qq, Zp + (2 * NG + g) * kST + qq);
    }
    __syncthreads();
    const int rows = (C + 31) / 32;                      // LINEAR packing: identity rows, ceil(C / 32) tiles, one K step
    if (wave < rows) {
      uint4 w[3];
      load_w(w, a.in_w, 1, 0);
      zero_acc();
      if (nb * 32 < W0) mma_step(w, Zp, kST, 0, 0);        // a wave whose 32 columns are all past the new ones has nothing to compute
      float* h0 = a.hist + item + p0 + q;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (co < C && q < W0) {
          const float u = acc[r] + a.in_b[co];
          h0[(int64_t)co * cap] = u / (1.f + expf(-u));
        }
      }
    }
    __syncthreads();                                     // level 0 is read back below; Zp is reused
    for (int i = tid; i < 3 * 2 * kST; i += NTHR) {      // Zp held the raw input: clear the two groups again (channel-padded rows stay zero)
      const int p = i / (2 * kST), rem = i - p * (2 * kST);
      Zp[(p * NG + rem / kST) * kST + rem % kST] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- the blocks.  Weight stream as in wavenet_fused_kernel: K-step index k = block * LS + s, register set k % (kSPD + 1)
  uint4 wa[kSPD + 1][3];
  auto fetch = [&](uint4 (&dst)[3], int block, int s) {
    const int bl = min(block, a.L - 1);
    if (s < GS) load_w(dst, a.gate_w[bl], GS, s);
    else load_w(dst, a.rs_w[bl], RS, s - GS);
  };
#pragma unroll
  for (int d = 0; d < kSPD; ++d) fetch(wa[d], 0, d);

  for (int blk = 0; blk < nblk; ++blk) {
    const int dil = a.cycle ? 1 << (blk % a.cycle) : 1;
    const float* gb = a.gate_b[blk];
    const float* rb = a.rs_b[blk];
    const int p = PREV(blk + 1), W = NEXT(blk + 1) - p;        // new columns [p, p + W) of level blk + 1
    const int valid = NEXT(blk);                                // level blk holds columns [0, valid)
    // Only the 32-column blocks that hold new columns are computed (a 30-frame push: one of three); `active` is uniform per wave and
    // mma_step contains no barrier.  The window is staged as far as the active waves read it.
    const bool active = nb * 32 < W;
    const int jend = min(kSXS, ((W + 31) & ~31) + 2 * kSH);
    // stage the window [p - kSH, p + kST + kSH) of level blk: one (8-channel group, column) unit per thread
    const float* xin = a.hist + (int64_t)blk * lvl + item;
    for (int i = tid; i < NG * kSXS; i += NTHR) {
      const int g = i / kSXS, j = i - g * kSXS;
      if (j >= jend) continue;
      const int t = p - kSH + j;
      const bool in = t >= 0 && t < valid;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        v[e] = (c < C && in) ? xin[(int64_t)c * cap + t] : 0.f;
      }
      if (j >= kSH && j < kSH + kST) {
#pragma unroll
        for (int e = 0; e < 8; ++e) Xf[(8 * g + e) * kST + j - kSH] = v[e];
      }
      s_split8_store(v, Xp + (0 * NG + g) * kSXS + j, Xp + (1 * NG + g) * kSXS + j, Xp + (2 * NG + g) * kSXS + j);
    }
    __syncthreads();
    // gated dilated conv: chunk-major, tap-minor (pack_conv's step order)
    zero_acc();
#pragma unroll
    for (int s = 0; s < GS; ++s) {
      const int ns = s + kSPD;
      fetch(wa[ns % (kSPD + 1)], ns < LS ? blk : blk + 1, ns < LS ? ns : ns - LS);
      if (active) mma_step(wa[s % (kSPD + 1)], Xp, kSXS, s / 3, kSH + (s % 3 - 1) * dil);
    }
    // z = sigmoid(gate) * tanh(filter)                                        (wavenet.py:129-130)
#pragma unroll
    for (int r = 0; r < 16; r += 8) {
      const int rho0 = 8 * (r >> 2) + 4 * h;
      const int c0 = wave * 16 + ((rho0 >> 3) >> 1) * 8 + (rho0 & 7);
      if (c0 < C) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v0 = acc[r + e] + gb[wave * 32 + rho0 + e];
          const float v1 = acc[(r + e + 4) & 15] + gb[wave * 32 + rho0 + e + 8];
          v[e] = (q < W && c0 + e < C) ? (1.f / (1.f + expf(-v0))) * tanhf(v1) : 0.f;
        }
        s_split4_store(v, slot(Zp, kST, 0, c0, q), slot(Zp, kST, 1, c0, q), slot(Zp, kST, 2, c0, q));
      }
    }
    __syncthreads();
    // residual / skip projection (1x1)                                         (wavenet.py:131-134)
    zero_acc();
#pragma unroll
    for (int s = 0; s < RS; ++s) {
      const int ks = GS + s, ns = ks + kSPD;
      fetch(wa[ns % (kSPD + 1)], ns < LS ? blk : blk + 1, ns < LS ? ns : ns - LS);
      if (active) mma_step(wa[ks % (kSPD + 1)], Zp, kST, s, 0);
    }
    float* xo = a.hist + (int64_t)(blk + 1) * lvl + item + p + q;
    float* so = a.skip + item + p + q;
#pragma unroll
    for (int r = 0; r < 16; r += 8) {
      const int rho0 = 8 * (r >> 2) + 4 * h;
      const int c0 = wave * 16 + ((rho0 >> 3) >> 1) * 8 + (rho0 & 7);
      if (c0 < C && q < W) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (c0 + e >= C) continue;
          const float v0 = acc[r + e] + rb[wave * 32 + rho0 + e];
          const float v1 = acc[(r + e + 4) & 15] + rb[wave * 32 + rho0 + e + 8];
          const int64_t o = (int64_t)(c0 + e) * cap;
          xo[o] = (Xf[(c0 + e) * kST + q] + v0) / 1.41421356237309504880f;
          so[o] = blk == 0 ? v1 : so[o] + v1;
        }
      }
    }
    __syncthreads();        // the stores above are read back by the next block's window (and by the tail); Xp / Xf / Zp are reused
  }

  // ---- skip_projection(sum of skips / sqrt(L)) on the columns whose sum is complete      (wavenet.py:218-219), masked store
  const int pL = PREV(a.L), WL = NEXT(a.L) - pL;
  if (WL <= 0) return;
  {
    const float* sb = a.skip + item + pL;
    for (int i = tid; i < NG * kST; i += NTHR) {
      const int g = i / kST, qq = i - g * kST;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        v[e] = (c < C && qq < WL) ? sb[(int64_t)c * cap + qq] * a.skip_scale : 0.f;
      }
      s_split8_store(v, Zp + (0 * NG + g) * kST + qq, Zp + (1 * NG + g) * kST + qq, Zp + (2 * NG + g) * kST + qq);
    }
  }
  __syncthreads();
  const int rows = (C + 31) / 32;
  if (wave < rows) {
    zero_acc();
    uint4 w[2][3];
    load_w(w[0], a.skip_w, RS, 0);
#pragma unroll
    for (int s = 0; s < RS; ++s) {
      if (s + 1 < RS) load_w(w[(s + 1) & 1], a.skip_w, RS, s + 1);
      if (nb * 32 < WL) mma_step(w[s & 1], Zp, kST, s, 0);
    }
    float* yb = a.y + item + pL + q;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co >= C) continue;
      const float bias = a.skip_b[co];
      if (q < WL) yb[(int64_t)co * cap] = pL + q < olim ? acc[r] + bias : 0.f;
    }
  }
}

template <int NCH, bool ITEMS> int launch_stream_t(const StreamArgs& a, hipStream_t st) {
  constexpr int NG = 2 * NCH, CP = 16 * NCH;
  constexpr size_t lds = (size_t)3 * NG * (kSXS + kST) * 16 + (size_t)CP * kST * 4;
  static bool raised = false;
  if (!raised && lds > 64 * 1024) {
    DMEL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&wavenet_stream_kernel<NCH, ITEMS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((wavenet_stream_kernel<NCH, ITEMS>), dim3((unsigned)a.N), dim3(192 * NCH), lds, st, a);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

__global__ void shift_lengths_kernel(const int64_t* len, int64_t shift, int64_t* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = max(len[i] - shift, (int64_t)0);
}

}  // namespace

int launch_shift_lengths(const int64_t* len, int64_t shift, int64_t* out, int n, hipStream_t st) {
  hipLaunchKernelGGL(shift_lengths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, len, shift, out, n);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// One sub-step of one row of frontiers: from cur[] towards next[], at most kST new columns per level.  A level may only run up to
// `dilation` columns behind its input's frontier -- unless that frontier is the end of the sequence (final step: next[l] == next[0] for
// every l), where the zero padding is real.  mid[]: the frontiers after the sub-step; *nblk: blocks 0 .. *nblk - 1 have new columns.
// Returns whether any level advances.
static bool stream_substep(const WaveNetFused& f, const int64_t* next, const int64_t* cur, int64_t* mid, int* nblk) {
  const bool final_step = next[f.L] == next[0];
  const int64_t total = next[0];
  bool any = false;
  *nblk = 0;
  for (int l = 0; l <= f.L; ++l) {
    int64_t lim = std::min(next[l], cur[l] + kST);
    if (l > 0) {
      const int dil = f.cycle ? 1 << ((l - 1) % f.cycle) : 1;
      lim = std::min(lim, (final_step && mid[l - 1] == total) ? total : mid[l - 1] - dil);
    }
    mid[l] = std::max(cur[l], lim);
    if (mid[l] > cur[l]) { any = true; if (l > 0) *nblk = l; }
  }
  return any;
}

static int stream_args(StreamArgs& a, const WaveNetFused& f, const float* x, float* hist, float* skip, float* y, const int64_t* out_len,
                       int len_div, int N, int64_t cap) {
  a.x = x; a.hist = hist; a.skip = skip; a.y = y; a.out_len = out_len; a.len_div = len_div > 0 ? len_div : 1;
  a.N = N; a.Cin = f.Cin; a.C = f.C; a.L = f.L; a.cycle = f.cycle; a.has_in = f.has_in; a.cap = cap;
  a.skip_scale = f.skip_scale;
  a.in_w = f.in_w; a.in_b = f.in_b; a.skip_w = f.skip_w; a.skip_b = f.skip_b;
  a.gate_w = reinterpret_cast<const void* const*>(f.table.p);
  a.gate_b = reinterpret_cast<const float* const*>(reinterpret_cast<const char*>(f.table.p) + (size_t)f.L * sizeof(void*));
  a.rs_w = reinterpret_cast<const void* const*>(reinterpret_cast<const char*>(f.table.p) + (size_t)2 * f.L * sizeof(void*));
  a.rs_b = reinterpret_cast<const float* const*>(reinterpret_cast<const char*>(f.table.p) + (size_t)3 * f.L * sizeof(void*));
  if (f.L > kStreamMaxL || cap >= ((int64_t)1 << 30)) { set_error("wavenet_stream: %d blocks / %lld columns out of range", f.L, (long long)cap); return DMEL_EUNSUPPORTED; }
  return DMEL_OK;
}

template <bool ITEMS> static int launch_stream(const StreamArgs& a, hipStream_t st) {
  switch ((a.C + 15) / 16) {
    case 5: return launch_stream_t<5, ITEMS>(a, st);
    case 4: return launch_stream_t<4, ITEMS>(a, st);
    case 3: return launch_stream_t<3, ITEMS>(a, st);
    // not reachable: WaveNetFused::ok (modules.hip, the caller's condition) admits 32 < C <= 80 only, i.e. nch 3 .. 5
    default: set_error("wavenet_stream: %d channels not instantiated", a.C); return DMEL_EUNSUPPORTED;
  }
}

// algorithmic flops / bytes of one item advancing from cur[] to mid[]
static void stream_cost(const WaveNetFused& f, const int64_t* cur, const int64_t* mid, double* flops, double* bytes) {
  int64_t cols = 0;
  for (int l = 1; l <= f.L; ++l) cols += mid[l] - cur[l];
  *flops = 2.0 * ((double)cols * (2.0 * f.C * 3 * f.C + 2.0 * f.C * f.C) + (double)(mid[f.L] - cur[f.L]) * f.C * f.C +
                  (f.has_in ? (double)(mid[0] - cur[0]) * f.C * f.Cin : 0.0));
  *bytes = 4.0 * (double)f.C * (3.0 * cols + 2.0 * kSH * f.L);
}

int launch_wavenet_stream(const WaveNetFused& f, const float* x, float* hist, float* skip, float* y, const int64_t* out_len, int len_div,
                          int N, int64_t cap, const int64_t* prev, const int64_t* next, hipStream_t st) {
  StreamArgs a{};
  DMEL_TRY(stream_args(a, f, x, hist, skip, y, out_len, len_div, N, cap));
  // Cut the step into sub-steps of at most kST new columns per level.
  int64_t cur[kStreamMaxL + 1];
  for (int l = 0; l <= f.L; ++l) cur[l] = prev[l];
  for (;;) {
    int64_t mid[kStreamMaxL + 1];
    if (!stream_substep(f, next, cur, mid, &a.nblk)) break;
    for (int l = 0; l <= f.L; ++l) { a.prev[l] = (int)cur[l]; a.next[l] = (int)mid[l]; }
    double flops, bytes;
    stream_cost(f, cur, mid, &flops, &bytes);
    {
      ProfScope ps("conv_igemm", st, N * flops, N * bytes, 6.0 * N * flops);
      DMEL_TRY(launch_stream<false>(a, st));
    }
    for (int l = 0; l <= f.L; ++l) cur[l] = mid[l];
  }
  for (int l = 0; l <= f.L; ++l)
    if (cur[l] != next[l]) { set_error("wavenet_stream: level %d cannot reach %lld from %lld", l, (long long)next[l], (long long)cur[l]); return DMEL_EINVAL; }
  return DMEL_OK;
}

// Per-utterance rows.  All sub-steps are planned on the host first -- a row that cannot reach its frontiers is refused before anything is
// launched -- then every sub-step is one table upload (launch arguments: the host tables are not read after this returns) and one launch
// over all N items; a row that is done is marked idle.  Launches on one stream run in order, so the one table is rewritten in place.
int launch_wavenet_stream_items(const WaveNetFused& f, const float* x, float* hist, float* skip, float* y, const int64_t* out_len, int len_div,
                                int N, int64_t cap, const int64_t* prev, const int64_t* next, int32_t* tab_dev, hipStream_t st) {
  StreamArgs a{};
  DMEL_TRY(stream_args(a, f, x, hist, skip, y, out_len, len_div, N, cap));
  a.tab = tab_dev;
  const int R = N / a.len_div, L1 = f.L + 1, RI = kStreamRowInts(f.L);
  std::vector<int64_t> cur(prev, prev + (size_t)R * L1);
  std::vector<int32_t> plan;                 // sub-step major: R rows of RI ints each
  std::vector<double> cost;                  // flops, bytes per sub-step, summed over the rows (x len_div items)
  for (;;) {
    bool any = false;
    const size_t base = plan.size();
    plan.resize(base + (size_t)R * RI);
    double fl = 0.0, by = 0.0;
    for (int r = 0; r < R; ++r) {
      int64_t mid[kStreamMaxL + 1];
      int nblk;
      int64_t* c = cur.data() + (size_t)r * L1;
      int32_t* t = plan.data() + base + (size_t)r * RI;
      const bool adv = stream_substep(f, next + (size_t)r * L1, c, mid, &nblk);
      for (int l = 0; l < L1; ++l) { t[l] = (int32_t)c[l]; t[L1 + l] = (int32_t)(adv ? mid[l] : c[l]); }
      t[2 * L1] = adv ? nblk : -1;
      if (!adv) continue;
      any = true;
      double f1, b1;
      stream_cost(f, c, mid, &f1, &b1);
      fl += a.len_div * f1; by += a.len_div * b1;
      for (int l = 0; l < L1; ++l) c[l] = mid[l];
    }
    if (!any) { plan.resize(base); break; }
    cost.push_back(fl); cost.push_back(by);
  }
  for (int r = 0; r < R; ++r)
    for (int l = 0; l < L1; ++l)
      if (cur[(size_t)r * L1 + l] != next[(size_t)r * L1 + l]) {
        set_error("wavenet_stream: utterance %d: level %d cannot reach %lld from %lld", r, l, (long long)next[(size_t)r * L1 + l],
                  (long long)cur[(size_t)r * L1 + l]);
        return DMEL_EINVAL;
      }
  const size_t steps = plan.size() / ((size_t)R * RI);
  for (size_t s = 0; s < steps; ++s) {
    DMEL_TRY(launch_table_put(plan.data() + s * R * RI, (size_t)R * RI * sizeof(int32_t), tab_dev, st));
    ProfScope ps("conv_igemm", st, cost[2 * s], cost[2 * s + 1], 6.0 * cost[2 * s]);
    DMEL_TRY(launch_stream<true>(a, st));
  }
  return DMEL_OK;
}

}  // namespace dmel
