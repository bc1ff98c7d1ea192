// Anti-aliased Snake / SnakeBeta activation, fused, for gfx950.
//
// Replaces the reference's CUDA kernel (alias_free_activation/cuda/anti_alias_activation_cuda.cu:44-179) and the
// six-launch torch path (alias_free_activation/torch/act.py:25-30, resample.py:29-38, filter.py:94-101):
//   x2 upsample (replicate pad 5/5, zero-stuffed 12-tap kaiser-sinc, x2 gain, crop 15/15)
//   -> v + 1/(beta+1e-9) * sin^2(alpha v) -> replicate pad 5/6 -> 12-tap low-pass, stride 2.
//
// Polyphase form (no zero stuffing): with f the 12 taps,
//   up[2m]   = 2 * sum_j f[2j+1] * x[clamp(m+2-j)]      j = 0..5
//   up[2m+1] = 2 * sum_j f[2j]   * x[clamp(m+3-j)]
//   out[t]   = sum_k f[k] * v[clamp(2t+k-5, 0, 2T-1)],  v = snake(up)
// One workgroup owns up to 1024 consecutive outputs of one (b, c) row: the row segment (+6/+6 halo) is read
// from HBM once with coalesced dword loads into LDS, the activated 2x signal lives only in LDS as
// (even, odd) pairs, and the store is coalesced.  HBM traffic = 1 read + 1 write per element, which is the
// algorithmic minimum (8 B/element); the reference kernel's stride-32-per-thread addressing is uncoalesced.
// Measured (rocprofv3 --pmc, round 1): ~120 vector instructions per output and VALU active ~100 % of the kernel, i.e.
// the kernel is VALU-issue bound at 2.3-2.6 TB/s, not HBM bound; the two sin^2 per input sample are a third of it.
#include "ops.h"
#include "snake_dev.h"

namespace dmel {

constexpr int kSnakeTile = 1024;

// 32-bit indices, and tiles that do not touch a sequence edge (block-uniform test) skip every clamp and select.
// (A v_pk_fma_f32 version of this kernel measured 0.6x: packed fp32 issues at half rate on gfx950.  Four consecutive samples
// per thread with ds_read_b128 windows -- 8 LDS reads instead of 56 per four outputs -- measured 0.84x: 2.26 vs 2.74 TB/s.)
// tu: the up-sampling taps times 2 (the x2 gain of UpSample1d, resample.py:37; exact in fp32), td: the low-pass taps of DownSample1d
// STAGED: xs was filled (and the workgroup synchronised) by the caller -- the software-pipelined kernel below
template <bool EDGE, bool STAGED = false>
__device__ __forceinline__ void aa_snake_tile(const float* __restrict__ xr, float* __restrict__ yr, const Taps12& tu, const Taps12& td,
                                              float a, float inv_b, int t0, int len, int T, float* xs, float2* vs, int tid) {
  if (!STAGED) {
    for (int i = tid; i < len + 12; i += 256) {
      int s = t0 - 6 + i;
      if (EDGE) s = min(max(s, 0), T - 1);
      xs[i] = xr[s];
    }
    __syncthreads();
  }
  for (int p = tid; p < len + 6; p += 256) {
    const int m = t0 - 3 + p;
    const int mc = EDGE ? min(max(m, 0), T - 1) : m;
    const float* xp = xs + (mc - t0 + 6);          // xp[d] = x[clamp(mc + d)]
    float ue = 0.f, uo = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      ue = fmaf(tu.f[2 * j + 1], xp[2 - j], ue);
      uo = fmaf(tu.f[2 * j], xp[3 - j], uo);
    }
    // both evaluations of sin^2 behind ONE wave-uniform test of the large-argument case: as two calls of sin_sq each is a basic block of
    // its own and the two 20-deep dependency chains run one after the other (snake_dev.h)
    float uu[2] = {ue, uo};
    const float aa[2] = {a, a}, bb[2] = {inv_b, inv_b};
    snake_n(uu, aa, bb);
    float ve = uu[0], vo = uu[1];
    if (EDGE) {
      if (m < 0) vo = ve;          // replicate pad of the 2x signal: v[0] on the left ...
      if (m > T - 1) ve = vo;      // ... v[2T-1] on the right
    }
    vs[p] = make_float2(ve, vo);
  }
  __syncthreads();
  for (int o = tid; o < len; o += 256) {
    float2 pv[7];
    lds_read7_b64(vs + o, pv);          // seven conflict-free ds_read_b64 (the compiler's six ds_read2_b32 were two-way conflicts each)
    const float2 p0 = pv[0], p1 = pv[1], p2 = pv[2], p3 = pv[3], p4 = pv[4], p5 = pv[5], p6 = pv[6];
    float acc = td.f[0] * p0.y;
    acc = fmaf(td.f[1], p1.x, acc);
    acc = fmaf(td.f[2], p1.y, acc);
    acc = fmaf(td.f[3], p2.x, acc);
    acc = fmaf(td.f[4], p2.y, acc);
    acc = fmaf(td.f[5], p3.x, acc);
    acc = fmaf(td.f[6], p3.y, acc);
    acc = fmaf(td.f[7], p4.x, acc);
    acc = fmaf(td.f[8], p4.y, acc);
    acc = fmaf(td.f[9], p5.x, acc);
    acc = fmaf(td.f[10], p5.y, acc);
    acc = fmaf(td.f[11], p6.x, acc);
    yr[t0 + o] = acc;
  }
}

__global__ __launch_bounds__(256) void aa_snake_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ alpha, const float* __restrict__ beta,
                                                          Taps12 tu, Taps12 td, int logscale, int C, int T, int nsub) {
  __shared__ float xs[kSnakeTile + 12];
  __shared__ float2 vs[kSnakeTile + 6];
  const int c = blockIdx.y, b = blockIdx.z;
  const float* xr = x + ((int64_t)b * C + c) * T;
  float* yr = y + ((int64_t)b * C + c) * T;
  float a = alpha[c], bt = beta ? beta[c] : a;
  if (logscale) {
    bt = beta ? expf(bt) : expf(a);
    a = expf(a);
  }
  const float inv_b = 1.0f / (bt + 1e-9f);
  // nsub consecutive tiles per workgroup, SOFTWARE-PIPELINED: the row segment of tile s + 1 is fetched into registers before tile s is
  // computed.  The kernel reads 4 KB per workgroup and then computes for ~4 us without touching memory: with 8 workgroups per CU only
  // ~10 KB per CU were in flight at any time, and bytes-in-flight / latency (Little's law: 10 KB / 2 us x 256 CUs = 1.3 TB/s) was
  // exactly the read rate the kernel achieved -- it was bound by memory-level parallelism, not by instruction issue.
  const int tid = threadIdx.x;
  constexpr int NR = (kSnakeTile + 12 + 255) / 256;
  float pre[NR];
  auto fetch = [&](int t0) {
    const int len = min(kSnakeTile, T - t0);
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int i = tid + 256 * k;
      const int sidx = min(max(t0 - 6 + min(i, len + 11), 0), T - 1);
      pre[k] = xr[sidx];
    }
  };
  const int first = blockIdx.x * nsub * kSnakeTile;
  if (first < T) fetch(first);
  for (int sub = 0; sub < nsub; ++sub) {
    const int t0 = first + sub * kSnakeTile;
    if (t0 >= T) break;
    const int len = min(kSnakeTile, T - t0);
    if (sub) __syncthreads();                  // the previous tile's reads of xs / vs are done
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int i = tid + 256 * k;
      if (i < len + 12) xs[i] = pre[k];
    }
    if (sub + 1 < nsub && t0 + kSnakeTile < T) fetch(t0 + kSnakeTile);     // in flight while this tile is computed
    __syncthreads();
    if (t0 >= 6 && t0 + len + 6 <= T) aa_snake_tile<false, true>(xr, yr, tu, td, a, inv_b, t0, len, T, xs, vs, tid);
    else aa_snake_tile<true, true>(xr, yr, tu, td, a, inv_b, t0, len, T, xs, vs, tid);
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------
// The reference has no backward for its fused kernel (alias_free_activation/cuda/activation1d.py:29-32 raises
// NotImplementedError; training goes through the six-op torch path and autograd).  Reverse mode of the forward above:
//   dv[i]   = sum_{t,k : clamp(2t+k-5) = i} f[k] dy[t]                      (transposed low-pass, replicate pads folded into the ends)
//   du      = dv * (1 + a * inv_b * sin(2 a u))                              (d/du [u + inv_b sin^2(a u)])
//   dx[s]   = sum_{m,j : clamp(m+2-j) = s} 2 f[2j+1] du_even[m] + sum_{m,j : clamp(m+3-j) = s} 2 f[2j] du_odd[m]
//   d a     = sum dv * inv_b * u * sin(2 a u),   d inv_b = sum dv * sin^2(a u)
// One workgroup owns the dx of up to 1024 samples of one (b, c) row, recomputes u from x (+6/+6 halo) and forms the two
// transposed filters by scatter-adding into LDS (ds_add_f32), which handles the replicate padding at the row ends with the same
// code as the interior.  Parameter gradients: block reduction, one atomic per workgroup.  Correctness first: this kernel has not
// been tuned (the vocoder is frozen in the reference's training_step; it matters for vocoder fine-tuning only).
// PARAMS = false is the frozen-vocoder form (dmel_bigvgan_backward_input): no dalpha / dbeta sums, no block reduction, no atomics to
// HBM -- dx goes through exactly the same operations, so it is bit-identical -- and the store may add up to two tensors of dx's shape:
// dx = (dx_act + radd) + racc.  radd is the residual branch of an AMP layer (x = xt + x); racc is the running sum over the blocks of a
// stage and may alias dx (every element is read and written by the same thread).
template <bool PARAMS>
__global__ __launch_bounds__(256) void aa_snake_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            float* dx, const float* __restrict__ alpha,
                                                            const float* __restrict__ beta, float* __restrict__ dalpha,
                                                            float* __restrict__ dbeta, const float* __restrict__ radd, const float* racc,
                                                            Taps12 tu, Taps12 td, int logscale, int C, int T) {
  __shared__ float xs[kSnakeTile + 12];
  __shared__ float dys[kSnakeTile + 12];
  __shared__ float dvs[2 * (kSnakeTile + 6)];
  __shared__ float dxs[kSnakeTile];
  __shared__ float red[2][4];
  const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int t0 = blockIdx.x * kSnakeTile;
  const int len = min(kSnakeTile, T - t0);
  const float* xr = x + ((int64_t)b * C + c) * T;
  const float* dyr = dy + ((int64_t)b * C + c) * T;
  float* dxr = dx + ((int64_t)b * C + c) * T;
  float a = alpha[c], bt = beta ? beta[c] : a;
  if (logscale) {
    bt = beta ? expf(bt) : expf(a);
    a = expf(a);
  }
  const float inv_b = 1.0f / (bt + 1e-9f);
  for (int i = tid; i < len + 12; i += 256) {
    const int s = t0 - 6 + i;
    xs[i] = xr[min(max(s, 0), T - 1)];
    dys[i] = (s >= 0 && s < T) ? dyr[s] : 0.f;
  }
  for (int i = tid; i < 2 * (len + 6); i += 256) dvs[i] = 0.f;
  for (int i = tid; i < len; i += 256) dxs[i] = 0.f;
  __syncthreads();
  // transposed low-pass: every dy sample in reach adds its 12 taps into the pairs this tile owns (m in [t0-3, t0+len+3)).  One tap per
  // round: within a round every sample writes a different element, so plain adds in a FIXED order replace atomics (dx is reproducible
  // bit for bit, and the same in both instantiations).  Taps that the replicate padding folds onto the row ends are left to one thread.
  auto near_end = [&](int v) { return v <= 2 || v >= T - 3; };
  for (int k = 0; k < 12; ++k) {
    for (int i = tid; i < len + 12; i += 256) {
      const int t = t0 - 6 + i;
      if (t < 0 || t >= T) continue;
      const int raw = 2 * t + k - 5;
      if (raw < 0 || raw > 2 * T - 1) continue;
      const int p = (raw >> 1) - (t0 - 3);
      if (p >= 0 && p < len + 6) dvs[2 * p + (raw & 1)] += td.f[k] * dys[i];
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (int t = 0; t < T; t = (t == 2 && T - 3 > 3) ? T - 3 : t + 1) {     // t = 0, 1, 2 and T-3, T-2, T-1, each once
      if (!near_end(t)) break;
      const int i = t - (t0 - 6);
      if (i < 0 || i >= len + 12) continue;
      for (int k = 0; k < 12; ++k) {
        const int raw = 2 * t + k - 5;
        if (raw >= 0 && raw <= 2 * T - 1) continue;
        const int vi = raw < 0 ? 0 : 2 * T - 1;
        const int p = (vi >> 1) - (t0 - 3);
        if (p >= 0 && p < len + 6) dvs[2 * p + (vi & 1)] += td.f[k] * dys[i];
      }
    }
  }
  __syncthreads();
  float sa = 0.f, sb = 0.f;
  for (int p = tid; p < len + 6; p += 256) {
    const int m = t0 - 3 + p;
    if (m < 0 || m > T - 1) continue;
    const float* xp = xs + (m - t0 + 6);          // xp[d] = x[clamp(m + d)] (xs holds the clamped row)
    float ue = 0.f, uo = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      ue = fmaf(tu.f[2 * j + 1], xp[2 - j], ue);
      uo = fmaf(tu.f[2 * j], xp[3 - j], uo);
    }
    const float dve = dvs[2 * p], dvo = dvs[2 * p + 1];
    const float s2e = sinf(2.f * a * ue), s2o = sinf(2.f * a * uo);
    const float due = dve * fmaf(a * inv_b, s2e, 1.f), duo = dvo * fmaf(a * inv_b, s2o, 1.f);
    if (PARAMS && m >= t0 && m < t0 + len) {      // parameter gradients: every pair is counted by exactly one tile
      sa += inv_b * (dve * ue * s2e + dvo * uo * s2o);
      sb += dve * sin_sq(a * ue) + dvo * sin_sq(a * uo);
    }
    dvs[2 * p] = due;                             // the pair is this thread's: du replaces dv in place
    dvs[2 * p + 1] = duo;
  }
  __syncthreads();
  // transposed up-sampler, the same way: one (tap, parity) per round, the folded ends by one thread
  for (int r = 0; r < 12; ++r) {
    const int j = r >> 1, odd = r & 1;
    const float coef = odd ? tu.f[2 * j] : tu.f[2 * j + 1];
    for (int p = tid; p < len + 6; p += 256) {
      const int m = t0 - 3 + p;
      if (m < 0 || m > T - 1) continue;
      const int sraw = m + 2 + odd - j;
      if (sraw < 0 || sraw > T - 1) continue;
      const int sl = sraw - t0;
      if (sl >= 0 && sl < len) dxs[sl] += coef * dvs[2 * p + odd];
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (int m = 0; m < T; m = (m == 2 && T - 3 > 3) ? T - 3 : m + 1) {
      if (!near_end(m)) break;
      const int p = m - (t0 - 3);
      if (p < 0 || p >= len + 6) continue;
      for (int r = 0; r < 12; ++r) {
        const int j = r >> 1, odd = r & 1;
        const int sraw = m + 2 + odd - j;
        if (sraw >= 0 && sraw <= T - 1) continue;
        const int sl = (sraw < 0 ? 0 : T - 1) - t0;
        if (sl >= 0 && sl < len) dxs[sl] += (odd ? tu.f[2 * j] : tu.f[2 * j + 1]) * dvs[2 * p + odd];
      }
    }
  }
  if (!PARAMS) {
    __syncthreads();
    const int64_t row = ((int64_t)b * C + c) * T + t0;
    for (int i = tid; i < len; i += 256) {
      float v = dxs[i];
      if (radd) v += radd[row + i];
      if (racc) v += racc[row + i];
      dxr[t0 + i] = v;
    }
    return;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sa += __shfl_xor(sa, o, 64);
    sb += __shfl_xor(sb, o, 64);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = sa; red[1][tid >> 6] = sb; }
  __syncthreads();
  for (int i = tid; i < len; i += 256) dxr[t0 + i] = dxs[i];
  if (tid == 0) {
    const float ga = red[0][0] + red[0][1] + red[0][2] + red[0][3];        // d loss / d a'      (a' = effective alpha)
    const float gib = red[1][0] + red[1][1] + red[1][2] + red[1][3];       // d loss / d inv_b
    const float gb = -inv_b * inv_b * gib;                                 // d loss / d b'      (inv_b = 1 / (b' + 1e-9))
    if (beta) {
      atomicAdd(&dalpha[c], logscale ? ga * a : ga);
      atomicAdd(&dbeta[c], logscale ? gb * bt : gb);
    } else {
      atomicAdd(&dalpha[c], logscale ? (ga + gb) * a : ga + gb);           // Snake: b' = a'
    }
  }
}

int launch_aa_snake_bwd(const float* x, const float* dy, float* dx, const float* alpha, const float* beta, float* dalpha, float* dbeta,
                        const float* up_taps_host, const float* down_taps_host, int logscale, int B, int C, int64_t T, hipStream_t s) {
  DMEL_CHECK_ARG(x && dy && dx && alpha && dalpha && up_taps_host && down_taps_host, "aa_snake_backward: NULL argument");
  DMEL_CHECK_ARG((beta != nullptr) == (dbeta != nullptr), "aa_snake_backward: dbeta must be given exactly when beta is");
  DMEL_CHECK_ARG(B > 0 && C > 0 && T > 0 && B <= 65535 && C <= 65535 && T < ((int64_t)1 << 29), "aa_snake_backward: bad shape");
  Taps12 tu, td;
  for (int i = 0; i < 12; ++i) { tu.f[i] = 2.f * up_taps_host[i]; td.f[i] = down_taps_host[i]; }
  DMEL_HIP(hipMemsetAsync(dalpha, 0, (size_t)C * sizeof(float), s));
  if (dbeta) DMEL_HIP(hipMemsetAsync(dbeta, 0, (size_t)C * sizeof(float), s));
  dim3 grid((unsigned)((T + kSnakeTile - 1) / kSnakeTile), (unsigned)C, (unsigned)B);
  {
    ProfScope ps("aa_snake_bwd", s, 0.0, 12.0 * (double)B * C * (double)T);
    hipLaunchKernelGGL(aa_snake_bwd_kernel<true>, grid, dim3(256), 0, s, x, dy, dx, alpha, beta, dalpha, dbeta, (const float*)nullptr,
                       (const float*)nullptr, tu, td, logscale, C, (int)T);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

int launch_aa_snake_bwd_input(const float* x, const float* dy, float* dx, const float* radd, const float* racc, const float* alpha,
                              const float* beta, const float* up_taps_host, const float* down_taps_host, int logscale, int B, int C,
                              int64_t T, hipStream_t s) {
  DMEL_CHECK_ARG(x && dy && dx && alpha && up_taps_host && down_taps_host, "aa_snake_backward_input: NULL argument");
  DMEL_CHECK_ARG(B > 0 && C > 0 && T > 0 && B <= 65535 && C <= 65535 && T < ((int64_t)1 << 29), "aa_snake_backward_input: bad shape");
  Taps12 tu, td;
  for (int i = 0; i < 12; ++i) { tu.f[i] = 2.f * up_taps_host[i]; td.f[i] = down_taps_host[i]; }
  dim3 grid((unsigned)((T + kSnakeTile - 1) / kSnakeTile), (unsigned)C, (unsigned)B);
  {
    ProfScope ps("aa_snake_bwd", s, 0.0, (12.0 + (radd ? 4.0 : 0.0) + (racc ? 4.0 : 0.0)) * (double)B * C * (double)T);
    hipLaunchKernelGGL(aa_snake_bwd_kernel<false>, grid, dim3(256), 0, s, x, dy, dx, alpha, beta, (float*)nullptr, (float*)nullptr, radd,
                       racc, tu, td, logscale, C, (int)T);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

int launch_aa_snake(const float* x, float* y, const float* alpha, const float* beta, const float* up_taps_host,
                    const float* down_taps_host, int logscale, int B, int C, int64_t T, hipStream_t s) {
  DMEL_CHECK_ARG(x && y && alpha && up_taps_host && down_taps_host, "aa_snake: NULL argument");
  DMEL_CHECK_ARG(B > 0 && C > 0 && T > 0 && B <= 65535 && C <= 65535 && T < ((int64_t)1 << 30), "aa_snake: bad shape");
  Taps12 tu, td;
  for (int i = 0; i < 12; ++i) { tu.f[i] = 2.f * up_taps_host[i]; td.f[i] = down_taps_host[i]; }
  // two tiles per workgroup (the second one's row segment is in flight while the first is computed): +4-8 % over one; four or eight
  // leave the last workgroup of a 5888- or 11776-sample row with a fraction of the work (measured 15-25 % slower on those rows)
  constexpr int nsub = 2;
  constexpr int tile = kSnakeTile * nsub;
  dim3 grid((unsigned)((T + tile - 1) / tile), (unsigned)C, (unsigned)B);
  {
    ProfScope ps("aa_snake", s, 0.0, 8.0 * (double)B * C * (double)T);
    hipLaunchKernelGGL(aa_snake_kernel, grid, dim3(256), 0, s, x, y, alpha, beta, tu, td, logscale, C, (int)T, nsub);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

}  // namespace dmel

extern "C" int dmel_aa_snake_backward_f32(const float* x, const float* dy, float* dx, const float* alpha, const float* beta,
                                          float* dalpha, float* dbeta, const float* up_filter12_host, const float* down_filter12_host,
                                          int logscale, int B, int C, int64_t T, void* stream) {
  return dmel::launch_aa_snake_bwd(x, dy, dx, alpha, beta, dalpha, dbeta, up_filter12_host, down_filter12_host, logscale, B, C, T,
                                   (hipStream_t)stream);
}

extern "C" int dmel_aa_snake_backward_input_f32(const float* x, const float* dy, const float* add /*nullable*/, float* dx, const float* alpha,
                                                const float* beta, const float* up_filter12_host, const float* down_filter12_host,
                                                int logscale, int B, int C, int64_t T, void* stream) {
  return dmel::launch_aa_snake_bwd_input(x, dy, dx, add, nullptr, alpha, beta, up_filter12_host, down_filter12_host, logscale, B, C, T,
                                         (hipStream_t)stream);
}

extern "C" int dmel_aa_snake_f32(const float* x, float* y, const float* alpha, const float* beta, const float* up_filter12_host,
                                 const float* down_filter12_host, int logscale, int B, int C, int64_t T, void* stream) {
  return dmel::launch_aa_snake(x, y, alpha, beta, up_filter12_host, down_filter12_host, logscale, B, C, T, (hipStream_t)stream);
}
