// Small HBM/launch-bound kernels of the quantiser path (a6-a8 of SURVEY.md section 8): depthwise conv + LayerNorm,
// FSQ encode / decode, masked copy, mask + quality add.  Their total work is ~0.02 GFLOP per utterance-second.
#include "ops.h"

namespace dmel {

// ---- ConvNeXt front half: depthwise k7 conv (zero pad 3) then LayerNorm over channels (eps, biased var).
// firefly.py:386-388 (dwconv, permute, norm).  x, y: (N, C, T).
constexpr int kDwTile = 32;

// ITEMS: row n is an item of lim = clamp(len[n / len_div], 0, T) columns with its own zero padding behind it: the taps read zero at or
// behind lim, y and h0 are zero there, and x is never read there (a neighbour's padding, NaN included, is harmless).  Columns in front
// of lim run the same fmaf chain as the plain kernel on a row of T = lim.  len / len_div are not read by the plain instantiation.
template <bool ITEMS>
__global__ __launch_bounds__(256) void dwconv_ln_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        const float* __restrict__ dw_w, const float* __restrict__ dw_b,
                                                        const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                        float* __restrict__ h0 /*nullable: pre-norm output, kept for training*/,
                                                        int C, int64_t T, float eps, const int64_t* __restrict__ len, int len_div) {
  extern __shared__ float sm[];
  float* hbuf = sm;                         // [C][kDwTile+1]
  float* stat = sm + (size_t)C * (kDwTile + 1);  // [2][kDwTile]
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int64_t t0 = (int64_t)blockIdx.x * kDwTile;
  const float* xn = x + (int64_t)n * C * T;
  int64_t lim = T;
  if constexpr (ITEMS) {
    lim = min(max(len[n / len_div], (int64_t)0), T);
    if (t0 >= lim) {      // the whole tile lies behind the item (uniform over the workgroup: in front of the first barrier)
      for (int idx = tid; idx < C * kDwTile; idx += 256) {
        const int c = idx / kDwTile, j = idx % kDwTile;
        const int64_t t = t0 + j;
        if (t < T) {
          y[((int64_t)n * C + c) * T + t] = 0.f;
          if (h0) h0[((int64_t)n * C + c) * T + t] = 0.f;
        }
      }
      return;
    }
  }
  for (int idx = tid; idx < C * kDwTile; idx += 256) {
    const int c = idx / kDwTile, j = idx % kDwTile;
    const int64_t t = t0 + j;
    float acc = 0.f;
    if (t < lim) {
      acc = dw_b[c];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int64_t s = t + k - 3;
        if (s >= 0 && s < lim) acc = fmaf(dw_w[c * 7 + k], xn[(int64_t)c * T + s], acc);
      }
    }
    hbuf[c * (kDwTile + 1) + j] = acc;
  }
  __syncthreads();
  if (tid < kDwTile) {
    float mean = 0.f;
    for (int c = 0; c < C; ++c) mean += hbuf[c * (kDwTile + 1) + tid];
    mean /= (float)C;
    float var = 0.f;
    for (int c = 0; c < C; ++c) {
      const float d = hbuf[c * (kDwTile + 1) + tid] - mean;
      var = fmaf(d, d, var);
    }
    var /= (float)C;
    stat[tid] = mean;
    stat[kDwTile + tid] = 1.0f / sqrtf(var + eps);
  }
  __syncthreads();
  float* yn = y + (int64_t)n * C * T;
  for (int idx = tid; idx < C * kDwTile; idx += 256) {
    const int c = idx / kDwTile, j = idx % kDwTile;
    const int64_t t = t0 + j;
    if (t < T) {
      if (ITEMS && t >= lim) {
        yn[(int64_t)c * T + t] = 0.f;
        if (h0) h0[((int64_t)n * C + c) * T + t] = 0.f;
        continue;
      }
      yn[(int64_t)c * T + t] = (hbuf[c * (kDwTile + 1) + j] - stat[j]) * stat[kDwTile + j] * ln_w[c] + ln_b[c];
      if (h0) h0[((int64_t)n * C + c) * T + t] = hbuf[c * (kDwTile + 1) + j];
    }
  }
}

int launch_dwconv_ln(const float* x, float* y, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b,
                     int N, int C, int64_t T, hipStream_t s, float* h0, const int64_t* len, int len_div) {
  DMEL_CHECK_ARG(N > 0 && N <= 65535 && C > 0 && T > 0, "dwconv_ln: bad shape");
  DMEL_CHECK_ARG(len == nullptr || (len_div > 0 && N % len_div == 0), "dwconv_ln: %d rows are no multiple of len_div = %d", N, len_div);
  const size_t lds = ((size_t)C * (kDwTile + 1) + 2 * kDwTile) * sizeof(float);
  DMEL_CHECK_ARG(lds <= 64 * 1024, "dwconv_ln: %d channels exceed the LDS tile", C);
  dim3 grid((unsigned)((T + kDwTile - 1) / kDwTile), (unsigned)N);
  {
    ProfScope ps("small", s, 0.0, 8.0 * N * C * (double)T);
    if (len)
      hipLaunchKernelGGL(dwconv_ln_kernel<true>, grid, dim3(256), lds, s, x, y, dw_w, dw_b, ln_w, ln_b, h0, C, T, 1e-6f, len, len_div);
    else
      hipLaunchKernelGGL(dwconv_ln_kernel<false>, grid, dim3(256), lds, s, x, y, dw_w, dw_b, ln_w, ln_b, h0, C, T, 1e-6f, len, 1);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- FSQ ---------------------------------------------------------------------------------------

__device__ __forceinline__ float fsq_bound(float z, const FsqConst& k, int j) {
  return tanhf(z + k.shift[j]) * k.half_l[j] - k.offset[j];
}

// z: (B*G, C, T4) channel-major rows of group g of item b at row b*G+g.  w_in: (G, D, C), b_in: (G, D).
// ids: (B, G, T4) int32.  prequant (optional): (G, B, T4, D).  len (nullable, B device int64): per-item token counts, clamped to [0, T4].
// Behind an item's count ids and prequant are written as 0 / 0.f.
__global__ __launch_bounds__(256) void fsq_encode_kernel(const float* __restrict__ z, const float* __restrict__ w_in,
                                                         const float* __restrict__ b_in, int32_t* __restrict__ ids,
                                                         float* __restrict__ prequant, FsqConst k, int B, int G, int C,
                                                         int64_t T4, const int64_t* __restrict__ len) {
  const int64_t total = (int64_t)B * G * T4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t l = i % T4;
  const int g = (int)((i / T4) % G);
  const int b = (int)(i / (T4 * G));
  if (len && l >= min(max(len[b], (int64_t)0), T4)) {      // items: behind item b's token count the id and prequant are 0 and z is not read
    ids[i] = 0;
    if (prequant)
      for (int j = 0; j < k.n_levels; ++j) prequant[(((int64_t)g * B + b) * T4 + l) * k.n_levels + j] = 0.f;
    return;
  }
  const float* zr = z + ((int64_t)(b * G + g) * C) * T4 + l;
  float acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = 0.f;
  for (int c = 0; c < C; ++c) {
    const float v = zr[(int64_t)c * T4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < k.n_levels) acc[j] = fmaf(w_in[((int64_t)g * k.n_levels + j) * C + c], v, acc[j]);
  }
  if (k.strict) {
    // strict mode: the last Linear and the bound(s) in float64, so that the value that is rounded does not depend on a summation
    // order or on a tanhf implementation -- two implementations fed the same features produce the same ids (the CPU oracle's strict
    // restatement does exactly this).  70 x 3 double FMAs per token: free.
    double dacc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
      const double v = (double)zr[(int64_t)c * T4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < k.n_levels) dacc[j] = fma((double)w_in[((int64_t)g * k.n_levels + j) * C + c], v, dacc[j]);
    }
    int sid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < k.n_levels) {
        double v = dacc[j] + (double)b_in[g * k.n_levels + j];
        const double hl = (double)k.half_l[j], of = (double)k.offset[j], sh = atanh(of / hl);   // shift in float64 too
        if (k.prebound) v = tanh(v + sh) * hl - of;
        v = tanh(v + sh) * hl - of;
        const float vf = (float)v;
        if (prequant) prequant[(((int64_t)g * B + b) * T4 + l) * k.n_levels + j] = vf;
        sid += ((int)rintf(vf) + k.half_width[j]) * k.basis[j];
      }
    }
    ids[i] = sid;
    return;
  }
  int id = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < k.n_levels) {
      float v = acc[j] + b_in[g * k.n_levels + j];
      if (k.prebound) v = fsq_bound(v, k, j);
      v = fsq_bound(v, k, j);
      if (prequant) prequant[(((int64_t)g * B + b) * T4 + l) * k.n_levels + j] = v;
      const int q = (int)rintf(v);  // round half to even, as torch.round
      id += (q + k.half_width[j]) * k.basis[j];
    }
  }
  ids[i] = id;
}

// ids (B, G, T4) -> z (B*G, C, T4):  code_j = (digit_j - hw_j) / hw_j ; z = W_out code + b_out.  w_out: (G, C, D).
// len (nullable, B device int64): per-item token counts, clamped to [0, T4].
__global__ __launch_bounds__(256) void fsq_decode_kernel(const int32_t* __restrict__ ids, const float* __restrict__ w_out,
                                                         const float* __restrict__ b_out, float* __restrict__ z, FsqConst k,
                                                         int B, int G, int C, int64_t T4, const int64_t* __restrict__ len) {
  const int64_t total = (int64_t)B * G * C * T4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t l = i % T4;
  const int c = (int)((i / T4) % C);
  const int64_t bg = i / (T4 * C);
  const int g = (int)(bg % G);
  if (len && l >= min(max(len[bg / G], (int64_t)0), T4)) {      // items: behind the item's token count z is 0.f and the id is not read
    z[i] = 0.f;
    return;
  }
  const int id = ids[bg * T4 + l];
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < k.n_levels) {
      const int digit = (id / k.basis[j]) % k.levels[j];
      const float code = ((float)digit - (float)k.half_width[j]) / (float)k.half_width[j];
      acc = fmaf(w_out[((int64_t)g * C + c) * k.n_levels + j], code, acc);
    }
  }
  z[i] = acc + b_out[g * C + c];
}

// ---- FSQ backward (straight-through estimator) -----------------------------------------------------------------------------
// forward (vector_quantize_pytorch FSQ.forward, restated): z3 = W_in x + b_in; [zz = bound(z3)]; b2 = bound(zz);
// code = round_ste(b2) / half_width; out = W_out code + b_out.  round_ste passes the gradient through unchanged, so
//   d b2 = d code / half_width;  d zz = d b2 * half_l (1 - tanh^2(zz + shift));  d z3 = the same factor once more when pre-bounded.
// Point kernel: one thread per (b, g, l): d x (70 channel rows) plus the per-point d z3 and code for the parameter kernel.
__global__ __launch_bounds__(256) void fsq_bwd_point_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                            const float* __restrict__ w_in, const float* __restrict__ b_in,
                                                            const float* __restrict__ w_out, float* __restrict__ dx,
                                                            float* __restrict__ dz3s, float* __restrict__ codes, FsqConst k, int B, int G,
                                                            int C, int64_t T4) {
  const int64_t total = (int64_t)B * G * T4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t l = i % T4;
  const int g = (int)((i / T4) % G);
  const int b = (int)(i / (T4 * G));
  const int64_t row0 = ((int64_t)(b * G + g) * C) * T4 + l;
  float z3[4], dcode[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { z3[j] = 0.f; dcode[j] = 0.f; }
  for (int c = 0; c < C; ++c) {
    const float v = x[row0 + (int64_t)c * T4], d = dout[row0 + (int64_t)c * T4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < k.n_levels) {
        z3[j] = fmaf(w_in[((int64_t)g * k.n_levels + j) * C + c], v, z3[j]);
        dcode[j] = fmaf(w_out[((int64_t)g * C + c) * k.n_levels + j], d, dcode[j]);
      }
  }
  float dz3[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    dz3[j] = 0.f;
    if (j < k.n_levels) {
      const float z = z3[j] + b_in[g * k.n_levels + j];
      float zz = z, f0 = 1.f;
      if (k.prebound) {
        const float t0 = tanhf(z + k.shift[j]);
        zz = t0 * k.half_l[j] - k.offset[j];
        f0 = k.half_l[j] * (1.f - t0 * t0);
      }
      const float t1 = tanhf(zz + k.shift[j]);
      const float b2 = t1 * k.half_l[j] - k.offset[j];
      const float code = rintf(b2) / (float)k.half_width[j];
      dz3[j] = dcode[j] / (float)k.half_width[j] * k.half_l[j] * (1.f - t1 * t1) * f0;
      const int64_t o = (((int64_t)g * B + b) * T4 + l) * k.n_levels + j;
      dz3s[o] = dz3[j];
      codes[o] = code;
    }
  }
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < k.n_levels) acc = fmaf(w_in[((int64_t)g * k.n_levels + j) * C + c], dz3[j], acc);
    dx[row0 + (int64_t)c * T4] = acc;
  }
}

// grid (C, G): d W_out[g][c][:], d b_out[g][c], d W_in[g][:][c] (and d b_in[g][:] from the c == 0 workgroup), reduced over (b, l)
__global__ __launch_bounds__(256) void fsq_bwd_param_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                            const float* __restrict__ dz3s, const float* __restrict__ codes,
                                                            float* __restrict__ dw_in, float* __restrict__ db_in, float* __restrict__ dw_out,
                                                            float* __restrict__ db_out, int D, int B, int G, int C, int64_t T4) {
  __shared__ float part[13][4];
  const int c = blockIdx.x, g = blockIdx.y;
  float acc[13];        // [0..3] dW_out, [4] db_out, [5..8] dW_in, [9..12] db_in
#pragma unroll
  for (int q = 0; q < 13; ++q) acc[q] = 0.f;
  const int64_t n_pts = (int64_t)B * T4;
  for (int64_t n = threadIdx.x; n < n_pts; n += 256) {
    const int b = (int)(n / T4);
    const int64_t l = n - (int64_t)b * T4;
    const int64_t e = ((int64_t)(b * G + g) * C + c) * T4 + l;
    const float d = dout[e], v = x[e];
    const int64_t o = (((int64_t)g * B + b) * T4 + l) * D;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < D) {
        acc[j] = fmaf(d, codes[o + j], acc[j]);
        acc[5 + j] = fmaf(dz3s[o + j], v, acc[5 + j]);
        acc[9 + j] += dz3s[o + j];
      }
    acc[4] += d;
  }
#pragma unroll
  for (int q = 0; q < 13; ++q) {
    float sacc = acc[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
    if ((threadIdx.x & 63) == 0) part[q][threadIdx.x >> 6] = sacc;
  }
  __syncthreads();
  if (threadIdx.x < 13) {
    const int q = threadIdx.x;
    const float v = part[q][0] + part[q][1] + part[q][2] + part[q][3];
    if (q < 4) { if (q < D) dw_out[((int64_t)g * C + c) * D + q] = v; }
    else if (q == 4) db_out[g * C + c] = v;
    else if (q < 9) { if (q - 5 < D) dw_in[((int64_t)g * D + (q - 5)) * C + c] = v; }
    else if (c == 0 && q - 9 < D) db_in[g * D + (q - 9)] = v;
  }
}

// dx (B*G, C, T4); parameter gradients in the packed (G, ...) layouts of the handle's FSQ buffers; scratch: 2 * G*B*T4*D floats
int launch_fsq_backward(const float* x, const float* dout, const float* w_in, const float* b_in, const float* w_out, float* dx,
                        float* dw_in, float* db_in, float* dw_out, float* db_out, float* scratch, const FsqConst& k, int B, int G, int C,
                        int64_t T4, hipStream_t s) {
  const int64_t total = (int64_t)B * G * T4;
  float* dz3s = scratch;
  float* codes = scratch + total * k.n_levels;
  hipLaunchKernelGGL(fsq_bwd_point_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, dout, w_in, b_in, w_out, dx, dz3s,
                     codes, k, B, G, C, T4);
  DMEL_HIP(hipGetLastError());
  hipLaunchKernelGGL(fsq_bwd_param_kernel, dim3((unsigned)C, (unsigned)G), dim3(256), 0, s, x, dout, dz3s, codes, dw_in, db_in, dw_out,
                     db_out, k.n_levels, B, G, C, T4);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

int make_fsq_const(FsqConst& k, const int* levels, int n, int prebound) {
  DMEL_CHECK_ARG(n >= 1 && n <= 4, "FSQ: 1..4 levels supported, got %d", n);
  k.n_levels = n;
  k.prebound = prebound;
  k.strict = 0;
  int basis = 1;
  for (int j = 0; j < 4; ++j) {
    if (j < n) {
      const int L = levels[j];
      DMEL_CHECK_ARG(L >= 2, "FSQ: level %d < 2", L);
      k.levels[j] = L;
      k.half_width[j] = L / 2;
      k.basis[j] = basis;
      basis *= L;
      k.half_l[j] = (float)(L - 1) * 1.001f / 2.0f;   // (levels - 1) * (1 + eps) / 2, eps = 1e-3, in fp32
      k.offset[j] = (L % 2 == 0) ? 0.5f : 0.0f;
      k.shift[j] = atanhf(k.offset[j] / k.half_l[j]);
    } else {
      k.levels[j] = 1; k.half_width[j] = 1; k.basis[j] = 0; k.half_l[j] = 0; k.offset[j] = 0; k.shift[j] = 0;
    }
  }
  return DMEL_OK;
}

int launch_fsq_encode(const float* z, const float* w_in, const float* b_in, int32_t* ids, float* prequant,
                      const FsqConst& k, int B, int G, int C, int64_t T4, hipStream_t s, const int64_t* len) {
  const int64_t total = (int64_t)B * G * T4;
  {
    ProfScope ps("small", s, 0.0, 4.0 * B * G * C * (double)T4);
    hipLaunchKernelGGL(fsq_encode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, z, w_in, b_in, ids,
                       prequant, k, B, G, C, T4, len);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

int launch_fsq_decode(const int32_t* ids, const float* w_out, const float* b_out, float* z, const FsqConst& k, int B,
                      int G, int C, int64_t T4, hipStream_t s, const int64_t* len) {
  const int64_t total = (int64_t)B * G * C * T4;
  {
    ProfScope ps("small", s, 0.0, 4.0 * (double)total);
    hipLaunchKernelGGL(fsq_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ids, w_out, b_out, z, k,
                       B, G, C, T4, len);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- y[n,c,t] = x[n,c,t] * (t < len[n / div])   (noise * mask of codec_lit_modules.py:473) ----------
__global__ __launch_bounds__(256) void masked_copy_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const int64_t* __restrict__ len, int div, int64_t CT, int64_t T,
                                                          int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = x[i];
  if (len) {
    const int64_t n = i / CT, t = i % T;
    if (t >= len[n / div]) v = 0.f;
  }
  y[i] = v;
}

int launch_masked_copy(const float* x, float* y, const int64_t* len, int div, int N, int C, int64_t T, hipStream_t s) {
  const int64_t total = (int64_t)N * C * T;
  {
    ProfScope ps("small", s, 0.0, 8.0 * (double)total);
    hipLaunchKernelGGL(masked_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, y, len,
                       div > 0 ? div : 1, (int64_t)C * T, T, total);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- folded batch: (N, C, T) <-> (C, N * P) with zero gaps (ops.h) -------------------------------------------------
__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ x, float* __restrict__ xf, const int64_t* __restrict__ len,
                                                   int div, int N, int C, int T, int P, int64_t pitch) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;      // column of the folded row
  const int c = blockIdx.y;
  if (j >= pitch) return;
  const int n = (int)(j / P), t = (int)(j - (int64_t)n * P);
  float v = 0.f;
  if (n < N && t < T && (!len || t < len[n / div])) v = x[((int64_t)n * C + c) * T + t];
  xf[(int64_t)c * pitch + j] = v;
}
__global__ __launch_bounds__(256) void unfold_kernel(const float* __restrict__ xf, float* __restrict__ y, const int64_t* __restrict__ len,
                                                     int div, int C, int T, int P, int64_t pitch, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % T);
  const int64_t nc = i / T;
  const int c = (int)(nc % C), n = (int)(nc / C);
  y[i] = (!len || t < len[n / div]) ? xf[(int64_t)c * pitch + (int64_t)n * P + t] : 0.f;
}

int launch_fold(const float* x, float* xf, const int64_t* len, int div, int N, int C, int64_t T, int P, int64_t pitch, hipStream_t s) {
  {
    ProfScope ps("small", s, 0.0, 4.0 * (double)N * C * T + 4.0 * (double)C * pitch);
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((pitch + 255) / 256), (unsigned)C), dim3(256), 0, s, x, xf, len, div > 0 ? div : 1, N, C,
                       (int)T, P, pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}
int launch_unfold(const float* xf, float* y, const int64_t* len, int div, int N, int C, int64_t T, int P, int64_t pitch, hipStream_t s) {
  const int64_t total = (int64_t)N * C * T;
  {
    ProfScope ps("small", s, 0.0, 8.0 * (double)total);
    hipLaunchKernelGGL(unfold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, xf, y, len, div > 0 ? div : 1, C, (int)T, P,
                       pitch, total);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- polyphase sinc resampling (torchaudio.functional.resample, the call of utils/spectrogram.py:122-123) ------------------------
// y[b, n * up + p] = sum_k bank[p][k] * xpad[b, n * down + k],  xpad = x padded with `width` zeros on the left and width + down on the
// right, k < kw = 2 * width + down.  One thread per output sample; the (up x kw) filter bank sits in LDS when it fits (16 kHz -> 24 kHz:
// 3 x 16 taps; 44.1 -> 24 kHz: 80 x 171), the input window comes through L1 (neighbouring outputs share all but `down` samples).
// HBM-bound: 4 bytes read per input + 4 written per output sample.
constexpr int kResampleLdsFloats = 15 * 1024;
// The taps of one output sample, shared by the whole-clip and the window launch so that both give an output the same bits: one fmaf per
// tap, k = 0 .. kw - 1 in order, zero for a tap outside the signal [0, L).  xb points at absolute sample `base` of the row.
__device__ __forceinline__ float resample_taps(const float* __restrict__ xb, int64_t base, const float* __restrict__ w, int64_t first,
                                               int64_t L, int kw) {
  float acc = 0.f;
  for (int k = 0; k < kw; ++k) {
    const int64_t s = first + k;
    const float v = (s >= 0 && s < L) ? xb[s - base] : 0.f;
    acc = fmaf(w[k], v, acc);
  }
  return acc;
}

// x (B, row_stride) holds the absolute samples [s0, ...) of a signal of L samples; the launch writes the absolute outputs
// [o0, o0 + n_out) to y (B, n_out).  The whole clip is (s0, o0, n_out) = (0, 0, Lout).  The host has checked that every tap inside
// [0, L) lies in the buffer (dmel_resample_window_f32).
// ITEMS (dmel_resample_window_items_f32): row b is a stream of its own, with its own window AND its own rate pair.  (s0, n_valid, o0,
// n_out, L, y_off, rate) are row blockIdx.y of `items`, (bank_off, down, up, width) row `rate` of `rates`; `bank` is then the arena
// all banks lie in, and item b's outputs go to y + b * y_row_stride + y_off.  Only where a workgroup finds its window, its bank and
// its store differs; the taps of an output do not.
constexpr int kResampleItemWords = 7, kResampleRateWords = 4;
// one int64 of a table row, read at the same address by every thread of the workgroup
__device__ __forceinline__ int64_t uniform_i64(const int64_t* p) {
  const int64_t v = *p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <bool ITEMS>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, int64_t row_stride, int64_t s0, float* __restrict__ y,
                                                       const float* __restrict__ bank, int64_t L, int64_t o0, int64_t n_out, int down,
                                                       int up, int width, int kw, int bank_in_lds, const int64_t* __restrict__ items,
                                                       const int64_t* __restrict__ rates, int64_t y_row_stride) {
  extern __shared__ float bsm[];
  int64_t y_at = (int64_t)blockIdx.y * n_out;                 // where the row's first output of this launch goes
  if constexpr (ITEMS) {
    const int64_t* it = items + kResampleItemWords * (int64_t)blockIdx.y;
    n_out = uniform_i64(it + 3);
    if ((int64_t)blockIdx.x * 256 >= n_out) return;           // workgroup-uniform, before the bank is staged and before the barrier
    s0 = uniform_i64(it);
    o0 = uniform_i64(it + 2);
    L = uniform_i64(it + 4);
    y_at = (int64_t)blockIdx.y * y_row_stride + uniform_i64(it + 5);
    const int64_t* rt = rates + kResampleRateWords * uniform_i64(it + 6);
    bank += uniform_i64(rt);
    down = (int)uniform_i64(rt + 1);
    up = (int)uniform_i64(rt + 2);
    width = (int)uniform_i64(rt + 3);
    kw = 2 * width + down;
    bank_in_lds = up * kw <= kResampleLdsFloats;              // the launch's LDS covers the largest bank that is staged
  }
  if (bank_in_lds) {
    for (int i = threadIdx.x; i < up * kw; i += 256) bsm[i] = bank[i];
    __syncthreads();
  }
  const float* bk = bank_in_lds ? bsm : bank;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  const int b = blockIdx.y;
  const int64_t o = o0 + i;
  const int64_t n = o / up;
  const int p = (int)(o - n * up);
  y[y_at + i] = resample_taps(x + (int64_t)b * row_stride, s0, bk + (int64_t)p * kw, n * down - width, L, kw);
}

int launch_resample_window(const float* x, int64_t row_stride, int64_t s0, int64_t n_samples, float* y, const float* bank_dev, int B,
                           int64_t L, int64_t o0, int64_t n_out, int down, int up, int width, hipStream_t s) {
  const int kw = 2 * width + down;
  const int in_lds = up * kw <= kResampleLdsFloats;
  {
    ProfScope ps("small", s, 0.0, 4.0 * (double)B * ((double)n_samples + (double)n_out));
    hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)((n_out + 255) / 256), (unsigned)B), dim3(256),
                       in_lds ? (size_t)up * kw * sizeof(float) : 0, s, x, row_stride, s0, y, bank_dev, L, o0, n_out, down, up, width, kw,
                       in_lds, nullptr, nullptr, 0);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// items / rates: the device tables the ITEMS kernel reads; max_out: the longest item's n_out; lds_floats: the largest staged bank
int launch_resample_window_items(const float* x, int64_t row_stride, float* y, int64_t y_row_stride, const float* arena_dev, int B,
                                 const int64_t* items_dev, const int64_t* rates_dev, int64_t max_out, int lds_floats, double bytes,
                                 hipStream_t s) {
  {
    ProfScope ps("small", s, 0.0, bytes);
    hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)((max_out + 255) / 256), (unsigned)B), dim3(256),
                       (size_t)lds_floats * sizeof(float), s, x, row_stride, 0, y, arena_dev, 0, 0, 0, 0, 0, 0, 0, 0, items_dev, rates_dev,
                       y_row_stride);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

int launch_resample(const float* x, float* y, const float* bank_dev, int B, int64_t L, int64_t Lout, int down, int up, int width,
                    hipStream_t s) {
  return launch_resample_window(x, L, 0, L, y, bank_dev, B, L, 0, Lout, down, up, width, s);
}

// ---- conv_post: C -> 1 channel, k taps, zero "same" padding, then tanh | clamp   (bigvgan.py:386-391) -----------
// One output row: a 32-row MFMA tile would be 97 % zeros, so this is a plain reduction over (channel, tap) -- HBM
// bound (C*T*4 bytes read per item, each input row read once per workgroup through L1).
constexpr int kPostTile = 1024;
// ITEMS: item b is a row of n = len[b] <= T columns inside the pitch T.  Taps at or beyond n read as zero (the item's own zero padding;
// nothing there is loaded), outputs in [n, T) are written as 0, and outputs in [0, n) are the bits of the plain form on the item alone.
template <bool ITEMS>
__global__ __launch_bounds__(256) void conv_post_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        const float* __restrict__ w, float bias, int C, int K, int T,
                                                        int act, const int64_t* __restrict__ len) {
  extern __shared__ float wsm[];   // [C][K]
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * kPostTile;
  const int n = ITEMS ? (int)min(max(len[b], (int64_t)0), (int64_t)T) : T;
  if (ITEMS && t0 >= n) {          // a tile wholly behind the item's end (block-uniform): zeros, no reduction
    for (int t = t0 + threadIdx.x; t < min(t0 + kPostTile, T); t += 256) y[(int64_t)b * T + t] = 0.f;
    return;
  }
  for (int i = threadIdx.x; i < C * K; i += 256) wsm[i] = w[i];
  __syncthreads();
  const float* xb = x + (int64_t)b * C * T;
  const int pad = (K - 1) / 2;
  float acc[4];
  int tt[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { acc[e] = bias; tt[e] = t0 + threadIdx.x + 256 * e; }
  for (int c = 0; c < C; ++c) {
    const float* xr = xb + (int64_t)c * T;
    for (int k = 0; k < K; ++k) {
      const float wv = wsm[c * K + k];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = tt[e] + k - pad;
        const float v = (s >= 0 && s < n) ? xr[s] : 0.f;
        acc[e] = fmaf(wv, v, acc[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (tt[e] < T) {
      const float v = act == 2 ? tanhf(acc[e]) : (act == 3 ? fminf(fmaxf(acc[e], -1.f), 1.f) : acc[e]);
      y[(int64_t)b * T + tt[e]] = (!ITEMS || tt[e] < n) ? v : 0.f;
    }
}

// len (nullable): B device int64, the per-item form
int launch_conv_post(const float* x, float* y, const float* w_dev, float bias, int act, int B, int C, int K, int64_t T,
                     hipStream_t s, const int64_t* len) {
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && K > 0 && (K % 2) == 1 && T > 0 && T < ((int64_t)1 << 30), "conv_post: bad shape");
  const size_t lds = (size_t)C * K * sizeof(float);
  DMEL_CHECK_ARG(lds <= 48 * 1024, "conv_post: weight table too large");
  dim3 grid((unsigned)((T + kPostTile - 1) / kPostTile), (unsigned)B);
  {
    ProfScope ps("small", s, 0.0, 4.0 * B * (double)T * (C + 1));
    if (len) hipLaunchKernelGGL(conv_post_kernel<true>, grid, dim3(256), lds, s, x, y, w_dev, bias, C, K, (int)T, act, len);
    else hipLaunchKernelGGL(conv_post_kernel<false>, grid, dim3(256), lds, s, x, y, w_dev, bias, C, K, (int)T, act, len);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// Backward-data of conv_post: dx[b,c,t] = sum_k w[c,k] g[b, t - k + K/2], g = dy * act'(y) with act' taken from the SAVED output y
// (tanh: 1 - y^2; clamp: 1 where |y| < 1, 0 where the output was clamped; none: 1).  One workgroup owns 1024 columns of one item: g
// (+ K-1 halo) is formed once in LDS, then every channel's row is K fmas per element and one coalesced store -- bound by the C*B*T write.
__global__ __launch_bounds__(256) void conv_post_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                            float* __restrict__ dx, const float* __restrict__ w, int C, int K, int T,
                                                            int act) {
  extern __shared__ float wsm[];   // [C][K] weights, then kPostTile + K - 1 values of g
  float* gs = wsm + C * K;
  for (int i = threadIdx.x; i < C * K; i += 256) wsm[i] = w[i];
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * kPostTile;
  const int pad = (K - 1) / 2;
  for (int i = threadIdx.x; i < kPostTile + K - 1; i += 256) {
    const int s = t0 - pad + i;
    float g = 0.f;
    if (s >= 0 && s < T) {
      const float yv = y ? y[(int64_t)b * T + s] : 0.f;
      const float d = act == 2 ? 1.f - yv * yv : (act == 3 ? (fabsf(yv) < 1.f ? 1.f : 0.f) : 1.f);
      g = dy[(int64_t)b * T + s] * d;
    }
    gs[i] = g;
  }
  __syncthreads();
  float* xb = dx + (int64_t)b * C * T;
  for (int c = 0; c < C; ++c) {
    const float* wc = wsm + c * K;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int lt = threadIdx.x + 256 * e;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(wc[k], gs[lt + K - 1 - k], acc);      // g[t - k + pad] sits at gs[(t - t0) + 2 pad - k]
      if (t0 + lt < T) xb[(int64_t)c * T + t0 + lt] = acc;
    }
  }
}

int launch_conv_post_bwd(const float* y, const float* dy, float* dx, const float* w_dev, int act, int B, int C, int K, int64_t T,
                         hipStream_t s) {
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && K > 0 && (K % 2) == 1 && T > 0 && T < ((int64_t)1 << 30), "conv_post_backward: bad shape");
  const size_t lds = ((size_t)C * K + kPostTile + K - 1) * sizeof(float);
  DMEL_CHECK_ARG(lds <= 48 * 1024, "conv_post_backward: weight table too large");
  dim3 grid((unsigned)((T + kPostTile - 1) / kPostTile), (unsigned)B);
  {
    ProfScope ps("small", s, 0.0, 4.0 * B * (double)T * (C + 2));
    hipLaunchKernelGGL(conv_post_bwd_kernel, grid, dim3(256), lds, s, y, dy, dx, w_dev, C, K, (int)T, act);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- z = z * mask + (w * value + bias)      codec_lit_modules.py:520-526 --------------------------
__global__ __launch_bounds__(256) void mask_add_quality_kernel(float* __restrict__ z, const int64_t* __restrict__ len,
                                                               const float* __restrict__ w, const float* __restrict__ bias,
                                                               float value, int C, int64_t T, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i % T;
  const int c = (int)((i / T) % C);
  const int64_t b = i / (T * C);
  float v = z[i];
  if (len && t >= len[b]) v = 0.f;
  z[i] = v + (w[c] * value + bias[c]);
}

// ---- data front end: peak-normalise + right-pad collate      dataset/lhotse_tts_dataset.py:29-32 (librosa.util.normalize(audio) * 0.95),
// :46-65 (right pad to the longest clip, stack to (B, 1, L), lengths (1, B) int32) ---------------------------------------------------------
// Clips stay where the decoder / resampler left them (B separate device buffers): pass 1 reduces max |x| per clip (slices of a clip on the
// grid, one atomic max on the bit pattern of a non-negative float per workgroup), pass 2 writes audios[b, 0, t] = x[t] / peak * 0.95 for
// t < len and 0 behind it, plus the lengths row.  librosa leaves a clip whose peak is below the smallest normal float unscaled.
constexpr int kCollateTile = 4096;
__global__ __launch_bounds__(256) void collate_absmax_kernel(const float* const* __restrict__ clips, const int64_t* __restrict__ lens,
                                                              const int32_t* __restrict__ order, uint32_t* __restrict__ peaks) {
  const int b = blockIdx.y;
  const int src = order ? order[b] : b;
  const int64_t n = lens[src];
  const int64_t t0 = (int64_t)blockIdx.x * kCollateTile;
  if (t0 >= n) return;
  const float* x = clips[src];
  float m = 0.f;
  for (int64_t t = t0 + threadIdx.x; t < min(n, t0 + kCollateTile); t += 256) m = fmaxf(m, fabsf(x[t]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(peaks + b, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}
__global__ __launch_bounds__(256) void collate_scale_pad_kernel(const float* const* __restrict__ clips, const int64_t* __restrict__ lens,
                                                                 const int32_t* __restrict__ order, const uint32_t* __restrict__ peaks,
                                                                 float* __restrict__ audios, int32_t* __restrict__ lengths, int64_t Lmax,
                                                                 float peak) {
  const int b = blockIdx.y;
  const int src = order ? order[b] : b;
  const int64_t n = min(lens[src], Lmax);
  if (blockIdx.x == 0 && threadIdx.x == 0) lengths[b] = (int32_t)n;
  const float* x = clips[src];
  const float m = __uint_as_float(peaks[b]);
  const float length = m < 1.17549435e-38f ? 1.0f : m;      // librosa.util.normalize: norms below `tiny` are replaced by 1 (fill = None)
  float* y = audios + (int64_t)b * Lmax;
  const int64_t t0 = (int64_t)blockIdx.x * kCollateTile;
  for (int64_t t = t0 + threadIdx.x; t < min(Lmax, t0 + kCollateTile); t += 256) y[t] = t < n ? (x[t] / length) * peak : 0.f;
}

}  // namespace dmel

extern "C" int dmel_collate_peak_f32(const float* const* clips_dev, const int64_t* lengths_dev, const int32_t* order_dev, float* audios,
                                     int32_t* audio_lengths, uint32_t* peaks_scratch, int B, int64_t Lmax, float peak, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(clips_dev && lengths_dev && audios && audio_lengths && peaks_scratch, "collate_peak: NULL argument");
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && Lmax > 0 && Lmax < ((int64_t)1 << 40), "collate_peak: bad shape");
  hipStream_t s = (hipStream_t)stream;
  DMEL_HIP(hipMemsetAsync(peaks_scratch, 0, (size_t)B * sizeof(uint32_t), s));
  const dim3 grid((unsigned)((Lmax + kCollateTile - 1) / kCollateTile), (unsigned)B);
  {
    ProfScope ps("small", s, 0.0, 12.0 * B * (double)Lmax);
    hipLaunchKernelGGL(collate_absmax_kernel, grid, dim3(256), 0, s, clips_dev, lengths_dev, order_dev, peaks_scratch);
    hipLaunchKernelGGL(collate_scale_pad_kernel, grid, dim3(256), 0, s, clips_dev, lengths_dev, order_dev, peaks_scratch, audios,
                       audio_lengths, Lmax, peak);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- host table -> device memory through launch arguments (common.h: launch_table_put) ------------------------------------------
constexpr int kPutWords = 448;      // 1792 bytes of the 4 KB an argument block may hold
struct PutChunk {
  uint32_t v[kPutWords];
};
__global__ __launch_bounds__(kPutWords) void table_put_kernel(PutChunk c, uint32_t* __restrict__ dst, int n) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = c.v[i];
}

int launch_table_put(const void* host, size_t bytes, void* dst_dev, hipStream_t st) {
  DMEL_CHECK_ARG(host && dst_dev && bytes % 4 == 0, "table_put: bad argument");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(host);
  uint32_t* dst = reinterpret_cast<uint32_t*>(dst_dev);
  for (size_t done = 0, words = bytes / 4; done < words; done += kPutWords) {
    const int n = (int)std::min<size_t>(kPutWords, words - done);
    PutChunk c;
    std::memcpy(c.v, src + done, (size_t)n * 4);
    std::memset(c.v + n, 0, (size_t)(kPutWords - n) * 4);
    hipLaunchKernelGGL(table_put_kernel, dim3(1), dim3(kPutWords), 0, st, c, dst + done, n);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- per-item column windows (conv.h ConvRun::win): the copies and lengths of the per-item layered streaming step ------------------
// dst[n][c][shift + q] = src[n][c][shift + q] for q < cols, shift / cols from row n / len_div of the table: what hipMemcpy2DAsync does for
// the lockstep step's one window.  The row is read at the same addresses by every thread of a workgroup.
__global__ __launch_bounds__(256) void copy_windows_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int64_t cap,
                                                           const int32_t* __restrict__ tab, int stride, int i_shift, int i_end, int len_div) {
  const int n = blockIdx.z, c = blockIdx.y;
  const int32_t* row = tab + (size_t)(n / len_div) * stride;
  const int shift = __builtin_amdgcn_readfirstlane(row[i_shift]);
  const int cols = __builtin_amdgcn_readfirstlane(row[i_end]) - shift;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= cols) return;
  const int64_t o = ((int64_t)n * C + c) * cap + shift + q;
  dst[o] = src[o];
}
int launch_copy_windows(const float* src, float* dst, int N, int C, int64_t cap, const int32_t* tab, int stride, int i_shift, int i_end,
                        int len_div, int64_t max_cols, int64_t cols_total, hipStream_t st) {
  DMEL_CHECK_ARG(src && dst && tab && N > 0 && N <= 65535 && C > 0 && C <= 65535 && max_cols > 0 && max_cols <= cap && len_div > 0 && stride > 0 &&
                     i_shift >= 0 && i_shift < stride && i_end >= 0 && i_end < stride, "copy_windows: bad argument");
  ProfScope ps("small", st, 0.0, 8.0 * C * (double)cols_total);
  hipLaunchKernelGGL(copy_windows_kernel, dim3((unsigned)((max_cols + 255) / 256), (unsigned)C, (unsigned)N), dim3(256), 0, st, src, dst, C, cap,
                     tab, stride, i_shift, i_end, len_div);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- ragged convert-copy over a pointer table (include/dmel_hip.h: dmel_pcm_convert_items) --------------------------------------------
// Item blockIdx.y is row (src, dst, n, word) of `items`; a workgroup owns FRAMES [2048 x, 2048 (x + 1)) of its item.  Every item has a
// mono f32 side and a wire side of c interleaved channels of format F (a DMEL_SAMPLE_* code), and one of two directions: IN, wire ->
// mono f32, and OUT, mono f32 -> wire.
// The rounding rule lives in these two functions and nowhere else: both paths of the kernel call them, so an element has the same bits on
// either.  s16 -> f32 is exact (|x| <= 2^15 times a power of two).  f32 -> s16: x 32768 is exact, the clamp comes first so that the
// conversion to int never sees a value out of range, rintf is v_rndne_f32 (nearest, ties to even, whatever the rounding mode); NaN -> 0.
constexpr int kPcmItemWords = 4, kPcmPerThread = 8, kPcmTile = 256 * kPcmPerThread;
__device__ __forceinline__ float pcm_s16_to_f32(int16_t v) { return (float)v * 0x1p-15f; }
__device__ __forceinline__ int16_t pcm_f32_to_s16(float v) {
  v = v != v ? 0.f : v;
  return (int16_t)(int)__builtin_rintf(fminf(fmaxf(v * 32768.f, -32768.f), 32767.f));
}
// G.711 (include/dmel_hip.h has the rule): 8-bit mu-law / A-law <-> the s16 value, integer arithmetic on every lane alike -- the segment
// is a count of leading zeros, never a search or a table, and the selects are v_cndmask, not branches.  x is an s16 value in an int.
__device__ __forceinline__ uint32_t g711_ulaw_encode(int x) {
  const int v = x >> 2;
  const bool neg = v < 0;
  const int m = min((neg ? -v : v) + 33, 8191);                 // 33 .. 8191: bit 5 is always set, so seg is 0 .. 7
  const int seg = 26 - __clz(m);                                // floor(log2 m) - 5
  return (uint32_t)(((seg << 4) | ((m >> (seg + 1)) & 15)) ^ (neg ? 0x7F : 0xFF));
}
__device__ __forceinline__ int g711_ulaw_decode(uint32_t code) {
  const uint32_t u = ~code & 0xFFu;
  const int t = (int)((((u & 15u) << 3) + 0x84u) << ((u & 0x70u) >> 4));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
__device__ __forceinline__ uint32_t g711_alaw_encode(int x) {
  const int v = x >> 3;
  const bool neg = v < 0;
  const int m = neg ? -v - 1 : v;                               // 0 .. 4095
  const int seg = max(27 - __clz(max(m, 1)), 0);                // max(floor(log2 max(m, 1)) - 4, 0): 0 .. 7
  const int mant = (m >> max(seg, 1)) & 15;                     // segments 0 and 1 both have a step of 2
  return (uint32_t)(((seg << 4) | mant) ^ (neg ? 0x55 : 0xD5));
}
__device__ __forceinline__ int g711_alaw_decode(uint32_t code) {
  const uint32_t a = (code ^ 0x55u) & 0xFFu;
  const int seg = (int)((a & 0x70u) >> 4);
  int t = (int)((a & 15u) << 4);
  t = seg == 0 ? t + 8 : (t + 0x108) << max(seg - 1, 0);
  return (a & 0x80u) ? t : -t;
}
// The four per-sample helpers.  The bits of a sample of format F (in the low end of a dword; what lies above them is ignored) as f32,
// and the bits of an f32 value in format F, by the rules above -- an f32 sample is its word, no arithmetic.
template <int F> constexpr int kPcmBytes = F == DMEL_SAMPLE_F32 ? 4 : F == DMEL_SAMPLE_S16 ? 2 : 1;
template <int F>
__device__ __forceinline__ float pcm_to_f32(uint32_t bits) {
  if constexpr (F == DMEL_SAMPLE_S16) return pcm_s16_to_f32((int16_t)bits);
  else if constexpr (F == DMEL_SAMPLE_ULAW) return (float)g711_ulaw_decode(bits) * 0x1p-15f;   // |x| < 2^15: exact
  else if constexpr (F == DMEL_SAMPLE_ALAW) return (float)g711_alaw_decode(bits) * 0x1p-15f;
  else return __uint_as_float(bits);
}
template <int F>
__device__ __forceinline__ uint32_t pcm_from_f32(float v) {
  if constexpr (F == DMEL_SAMPLE_F32) return __float_as_uint(v);
  else if constexpr (F == DMEL_SAMPLE_S16) return (uint32_t)(uint16_t)pcm_f32_to_s16(v);
  else if constexpr (F == DMEL_SAMPLE_ULAW) return g711_ulaw_encode(pcm_f32_to_s16(v));   // the s16 rounding rule, unchanged
  else return g711_alaw_encode(pcm_f32_to_s16(v));
}
// Sample i of w, and its store.  w is the wire itself (T is the format's own type, one sample each) or a thread's register dwords (T =
// uint32_t, 4 / kPcmBytes<F> samples each: i is then a constant of an unrolled loop, the shifts fold, and w starts as zeros for a put).
template <int F, typename T>
__device__ __forceinline__ uint32_t pcm_get(const T* w, int64_t i) {
  constexpr int kPer = sizeof(T) / kPcmBytes<F>;
  return (uint32_t)w[i / kPer] >> (8 * kPcmBytes<F> * (int)(i % kPer));
}
template <int F, typename T>
__device__ __forceinline__ void pcm_put(T* w, int64_t i, uint32_t bits) {
  constexpr int kPer = sizeof(T) / kPcmBytes<F>;
  if constexpr (kPer == 1) w[i] = (T)bits;
  else w[i / kPer] |= bits << (8 * kPcmBytes<F> * (int)(i % kPer));
}
// NW dwords between memory and registers: one 8-byte access (NW == 2) or NW / 4 16-byte accesses
template <int NW>
__device__ __forceinline__ void pcm_load(uint32_t* w, const void* p) {
  if constexpr (NW == 2) {
    const uint2 a = *static_cast<const uint2*>(p);
    w[0] = a.x; w[1] = a.y;
  } else {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) {
      const uint4 a = static_cast<const uint4*>(p)[q];
      w[4 * q] = a.x; w[4 * q + 1] = a.y; w[4 * q + 2] = a.z; w[4 * q + 3] = a.w;
    }
  }
}
template <int NW>
__device__ __forceinline__ void pcm_store(void* p, const uint32_t* w) {
  if constexpr (NW == 2) {
    *static_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) static_cast<uint4*>(p)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}
// The wide body: the 8 consecutive frames from frame e on, all inside the item, C = 1 or 2 channels.  On the f32 side they are two
// 16-byte accesses, on the wire side NW = 2, 4, 8 or 16 dwords, unpacked and packed in registers.  The stereo mean is acc = l; acc += r;
// acc / 2.0f -- a correctly rounded division whatever the compiler makes of it, so a frame has the bits the frame loop gives it.
template <int F, int C, bool IN>
__device__ __forceinline__ void pcm_wide(const void* src, void* dst, int64_t e, int pick) {
  constexpr int NW = kPcmPerThread * C * kPcmBytes<F> / 4;
  uint32_t w[NW], f[kPcmPerThread];
  if constexpr (IN) {
    pcm_load<NW>(w, static_cast<const uint8_t*>(src) + e * C * kPcmBytes<F>);
#pragma unroll
    for (int j = 0; j < kPcmPerThread; ++j) {
      float y = pcm_to_f32<F>(pcm_get<F>(w, C * j));
      if constexpr (C == 2) {
        const float l = y, r = pcm_to_f32<F>(pcm_get<F>(w, C * j + 1));
        if (pick < 0) {
          float acc = l;
          acc += r;
          y = acc / 2.0f;
        } else {
          y = pick ? r : l;
        }
      }
      f[j] = __float_as_uint(y);
    }
    pcm_store<kPcmPerThread>(static_cast<float*>(dst) + e, f);
  } else {
    pcm_load<kPcmPerThread>(f, static_cast<const float*>(src) + e);
#pragma unroll
    for (int j = 0; j < NW; ++j) w[j] = 0u;
#pragma unroll
    for (int j = 0; j < kPcmPerThread; ++j) {
      const uint32_t v = pcm_from_f32<F>(__uint_as_float(f[j]));
#pragma unroll
      for (int k = 0; k < C; ++k) pcm_put<F>(w, C * j + k, v);
    }
    pcm_store<NW>(static_cast<uint8_t*>(dst) + e * C * kPcmBytes<F>, w);
  }
}
// One item's tile.  IN: c channels of format F -> mono f32; pick = k: y = x_k, no arithmetic; pick < 0: acc = x_0; acc += x_1; ...;
// y = acc / (float)c, the IEEE division, in channel order.  OUT: the sample is converted ONCE and its bits are stored c times.  c, pick
// and `wide` are workgroup-uniform.  `wide`: c <= 2, the f32 side 16-byte aligned and the wire side aligned to what a thread moves at
// once -- 8 bytes for a mono law, 16 for everything else; then a thread whose 8 consecutive frames all lie in the item takes pcm_wide.
// Everything else -- another c, an unaligned item, the frames behind the last whole 8 -- goes frame by frame, frame e of the tile to
// thread e % 256 so that a wave still reads and writes consecutive addresses.
template <int F, bool IN>
__device__ __forceinline__ void pcm_tile_c(const void* src, void* dst, uint64_t sa, uint64_t da, int64_t n, int64_t base, int c, int pick) {
  using T = std::conditional_t<kPcmBytes<F> == 4, uint32_t, std::conditional_t<kPcmBytes<F> == 2, uint16_t, uint8_t>>;
  const bool wide = c <= 2 && ((IN ? da : sa) & 15) == 0 && ((IN ? sa : da) & (kPcmBytes<F> == 1 && c == 1 ? 7 : 15)) == 0;
  int64_t from = base;                                         // the frame-wise path covers [from, min(n, base + kPcmTile))
  if (wide) {
    const int64_t whole = base + (min(n - base, (int64_t)kPcmTile) & ~(int64_t)(kPcmPerThread - 1));
    const int64_t e = base + (int64_t)threadIdx.x * kPcmPerThread;
    if (e < whole) {
      if (c == 1) pcm_wide<F, 1, IN>(src, dst, e, pick);
      else pcm_wide<F, 2, IN>(src, dst, e, pick);
    }
    from = whole;
  }
  const int64_t end = min(n, base + kPcmTile);
  for (int64_t e = from + threadIdx.x; e < end; e += 256) {
    if constexpr (IN) {
      const T* s = static_cast<const T*>(src);
      float y;
      if (pick >= 0) {
        y = pcm_to_f32<F>(pcm_get<F>(s, e * c + pick));
      } else {
        float acc = pcm_to_f32<F>(pcm_get<F>(s, e * c));
        for (int j = 1; j < c; ++j) acc += pcm_to_f32<F>(pcm_get<F>(s, e * c + j));
        y = acc / (float)c;
      }
      static_cast<float*>(dst)[e] = y;
    } else {
      const uint32_t v = pcm_from_f32<F>(static_cast<const float*>(src)[e]);
      for (int j = 0; j < c; ++j) pcm_put<F>(static_cast<T*>(dst), e * c + j, v);
    }
  }
}
// The counts that have a wide body reach pcm_tile_c as literals, so that their frame loop is compiled for them as well: with a
// run-time c a mono item's loop keeps a multiply and an inner loop per frame, and an unaligned mono item of a million samples was
// measured 5 to 34 % slower for them.  A mono item runs as pick = 0: its sample is moved, never acc / 1.0f, which would quiet a
// signalling NaN (OUT ignores the pick).
template <int F, bool IN>
__device__ __forceinline__ void pcm_tile(const void* src, void* dst, uint64_t sa, uint64_t da, int64_t n, int64_t base, int c, int pick) {
  if (c == 1) pcm_tile_c<F, IN>(src, dst, sa, da, n, base, 1, 0);
  else if (c == 2) pcm_tile_c<F, IN>(src, dst, sa, da, n, base, 2, pick);
  else pcm_tile_c<F, IN>(src, dst, sa, da, n, base, c, pick);
}
// the switch on the wire format f, one per direction
template <bool IN>
__device__ __forceinline__ void pcm_tile_of(int f, const void* src, void* dst, uint64_t sa, uint64_t da, int64_t n, int64_t base, int c,
                                            int pick) {
  switch (f) {
    case DMEL_SAMPLE_S16: pcm_tile<DMEL_SAMPLE_S16, IN>(src, dst, sa, da, n, base, c, pick); break;
    case DMEL_SAMPLE_ULAW: pcm_tile<DMEL_SAMPLE_ULAW, IN>(src, dst, sa, da, n, base, c, pick); break;
    case DMEL_SAMPLE_ALAW: pcm_tile<DMEL_SAMPLE_ALAW, IN>(src, dst, sa, da, n, base, c, pick); break;
    default: pcm_tile<DMEL_SAMPLE_F32, IN>(src, dst, sa, da, n, base, c, pick); break;
  }
}
// The item's fourth word: src_fmt | dst_fmt << 8 | (src_ch - 1) << 16 | (dst_ch - 1) << 20 | (pick + 1) << 24 (the entry admits c -> 1
// and 1 -> c only, one side f32).  An item is OUT when its destination has channels or a format other than f32; mono f32 -> f32 is IN
// with F = f32.
__global__ __launch_bounds__(256) void pcm_convert_kernel(const int64_t* __restrict__ items) {
  const int64_t* it = items + kPcmItemWords * (int64_t)blockIdx.y;
  const int64_t n = uniform_i64(it + 2);
  const int64_t base = (int64_t)blockIdx.x * kPcmTile;
  if (base >= n) return;                                       // workgroup-uniform: every workgroup of an idle item leaves here
  const uint64_t sa = (uint64_t)uniform_i64(it), da = (uint64_t)uniform_i64(it + 1);
  const int64_t word = uniform_i64(it + 3);
  const int sf = (int)(word & 0xff), df = (int)((word >> 8) & 0xff);
  const int sc = (int)((word >> 16) & 7) + 1, dc = (int)((word >> 20) & 7) + 1, pick = (int)((word >> 24) & 15) - 1;
  const void* src = reinterpret_cast<const void*>(sa);
  void* dst = reinterpret_cast<void*>(da);
  if (dc > 1 || df != DMEL_SAMPLE_F32) pcm_tile_of<false>(df, src, dst, sa, da, n, base, dc, -1);
  else pcm_tile_of<true>(sf, src, dst, sa, da, n, base, sc, pick);
}

// out[r] = max(len[r] - row r's shift, 0): an item's output length relative to the first column of its window
__global__ void shift_lengths_items_kernel(const int64_t* __restrict__ len, const int32_t* __restrict__ tab, int stride, int i_shift,
                                           int64_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = max(len[i] - (int64_t)tab[(size_t)i * stride + i_shift], (int64_t)0);
}
int launch_shift_lengths_items(const int64_t* len, const int32_t* tab, int stride, int i_shift, int64_t* out, int n, hipStream_t st) {
  DMEL_CHECK_ARG(len && tab && out && n > 0 && stride > 0 && i_shift >= 0 && i_shift < stride, "shift_lengths_items: bad argument");
  hipLaunchKernelGGL(shift_lengths_items_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, len, tab, stride, i_shift, out, n);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// tab[i * n + b] = clamp(len[b], 0, T) * scale.v[i]: the items' lengths at every stage of an up-sampling stack, made on the device (no host
// read of the lengths, no synchronisation)
__global__ void length_tables_kernel(const int64_t* __restrict__ len, int64_t* __restrict__ tab, int n, int64_t T, int stages, LenScales scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const int64_t l = min(max(len[b], (int64_t)0), T);
  for (int i = 0; i < stages; ++i) tab[(size_t)i * n + b] = l * scale.v[i];
}
int launch_length_tables(const int64_t* len, int64_t* tab, int n, int64_t T, int stages, const LenScales& scale, hipStream_t st) {
  DMEL_CHECK_ARG(len && tab && n > 0 && T > 0 && stages > 0 && stages <= LenScales::kMax, "length_tables: bad argument");
  hipLaunchKernelGGL(length_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, len, tab, n, T, stages, scale);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// tab[i * n + b] = clamp(len[b], 0, T) >> i (down) or << i (up): the items' lengths at every stage of the quantiser's factor-2 down- or
// up-sampling stack.  The floors of the down form are those of the strided convolutions (7 -> 3 -> 1).  One thread per item.
__global__ void stage_lengths_kernel(const int64_t* __restrict__ len, int64_t* __restrict__ tab, int n, int64_t T, int stages, int down) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const int64_t l = min(max(len[b], (int64_t)0), T);
  for (int i = 0; i < stages; ++i) tab[(size_t)i * n + b] = down ? (l >> i) : (l << i);
}
int launch_stage_lengths(const int64_t* len, int64_t* tab, int n, int64_t T, int stages, int down, hipStream_t st) {
  DMEL_CHECK_ARG(len && tab && n > 0 && T > 0 && stages > 0 && stages <= 31, "stage_lengths: bad argument");
  hipLaunchKernelGGL(stage_lengths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, len, tab, n, T, stages, down);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

}  // namespace dmel

extern "C" int dmel_mask_add_quality_f32(float* z, const int64_t* lengths, const float* w, const float* bias, float value,
                                         int B, int C, int64_t T, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(z && w && bias && B > 0 && C > 0 && T > 0, "mask_add_quality: bad argument");
  const int64_t total = (int64_t)B * C * T;
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps("small", s, 0.0, 8.0 * (double)total);
    hipLaunchKernelGGL(mask_add_quality_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, z, lengths, w,
                       bias, value, C, T, total);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// ---- the FSQ kernels alone (include/dmel_hip.h: dmel_fsq_*_f32): the launchers above on caller-supplied packed parameters -------------
static int fsq_entry_const(dmel::FsqConst& k, const char* who, const int* levels, int n_levels, int prebound, int strict, int B, int G, int C,
                           int64_t T4) {
  DMEL_CHECK_ARG(levels && n_levels >= 1 && n_levels <= 4, "%s: 1..4 levels", who);
  DMEL_CHECK_ARG(B > 0 && G > 0 && C > 0 && T4 > 0 && (int64_t)B * G * C * T4 < ((int64_t)1 << 31) * 256, "%s: bad shape", who);
  int64_t codes = 1;
  for (int j = 0; j < n_levels; ++j) {
    DMEL_CHECK_ARG(levels[j] >= 2 && levels[j] <= 1024, "%s: level %d outside 2..1024", who, levels[j]);
    codes *= levels[j];
  }
  DMEL_CHECK_ARG(codes < ((int64_t)1 << 31), "%s: the codebook does not fit an int32 id", who);
  DMEL_TRY(dmel::make_fsq_const(k, levels, n_levels, prebound != 0));
  k.strict = strict != 0;
  return DMEL_OK;
}

extern "C" int dmel_fsq_encode_f32(const float* z, const float* w_in, const float* b_in, const int* levels, int n_levels, int prebound,
                                   int strict, const int64_t* lengths_dev, int32_t* ids, float* prequant, int B, int G, int C, int64_t T4,
                                   void* stream) {
  DMEL_CHECK_ARG(z && w_in && b_in && ids, "fsq_encode: NULL argument");
  dmel::FsqConst k;
  DMEL_TRY(fsq_entry_const(k, "fsq_encode", levels, n_levels, prebound, strict, B, G, C, T4));
  return dmel::launch_fsq_encode(z, w_in, b_in, ids, prequant, k, B, G, C, T4, (hipStream_t)stream, lengths_dev);
}

extern "C" int dmel_fsq_decode_f32(const int32_t* ids, const float* w_out, const float* b_out, const int* levels, int n_levels,
                                   const int64_t* lengths_dev, float* z, int B, int G, int C, int64_t T4, void* stream) {
  DMEL_CHECK_ARG(ids && w_out && b_out && z, "fsq_decode: NULL argument");
  dmel::FsqConst k;
  DMEL_TRY(fsq_entry_const(k, "fsq_decode", levels, n_levels, 0, 0, B, G, C, T4));
  return dmel::launch_fsq_decode(ids, w_out, b_out, z, k, B, G, C, T4, (hipStream_t)stream, lengths_dev);
}

extern "C" int dmel_fsq_backward_f32(const float* x, const float* dout, const float* w_in, const float* b_in, const float* w_out,
                                     const int* levels, int n_levels, int prebound, float* dx, float* dw_in, float* db_in, float* dw_out,
                                     float* db_out, float* scratch, size_t scratch_floats, int B, int G, int C, int64_t T4, void* stream) {
  DMEL_CHECK_ARG(x && dout && w_in && b_in && w_out && dx && dw_in && db_in && dw_out && db_out && scratch, "fsq_backward: NULL argument");
  dmel::FsqConst k;
  DMEL_TRY(fsq_entry_const(k, "fsq_backward", levels, n_levels, prebound, 0, B, G, C, T4));
  DMEL_CHECK_ARG(G <= 65535, "fsq_backward: %d groups exceed the grid", G);
  const size_t need = (size_t)2 * B * G * T4 * n_levels;
  DMEL_CHECK_ARG(scratch_floats >= need, "fsq_backward: scratch too small (%zu < %zu floats)", scratch_floats, need);
  return dmel::launch_fsq_backward(x, dout, w_in, b_in, w_out, dx, dw_in, db_in, dw_out, db_out, scratch, k, B, G, C, T4, (hipStream_t)stream);
}

extern "C" int dmel_resample_f32(const float* x, float* y, const float* filter_bank_dev, int B, int64_t L, int64_t Lout, int orig_freq,
                                 int new_freq, int width, void* stream) {
  DMEL_CHECK_ARG(x && y && filter_bank_dev, "resample: NULL argument");
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && Lout > 0 && orig_freq > 0 && new_freq > 0 && width >= 0, "resample: bad shape");
  DMEL_CHECK_ARG(Lout <= (L * new_freq + orig_freq - 1) / orig_freq, "resample: Lout exceeds ceil(new_freq * L / orig_freq)");
  return dmel::launch_resample(x, y, filter_bank_dev, B, L, Lout, orig_freq, new_freq, width, (hipStream_t)stream);
}

// ---- outputs of a window of a longer signal (include/dmel_hip.h: dmel_resample_window_f32) ----------------------------------------
// the window rules for one buffer [s0, s0 + n_samples) and one rate pair; *L_out: the signal length the kernel pads at.  who: "" or "item b: "
static int resample_window_check(int64_t n_samples, int64_t s0, int64_t o0, int64_t n_out, int64_t total_length, int64_t orig_freq,
                                 int64_t new_freq, int64_t width, const char* who, int64_t* L_out) {
  DMEL_CHECK_ARG(n_samples > 0 && s0 >= 0 && o0 >= 0 && n_out > 0, "resample_window: %sbad window", who);
  const bool known = total_length >= 0;
  const int64_t have_end = s0 + n_samples;                 // the buffer holds absolute samples [s0, have_end)
  DMEL_CHECK_ARG(have_end < ((int64_t)1 << 40) && o0 + n_out < ((int64_t)1 << 40), "resample_window: %sposition out of range", who);
  if (known) {
    DMEL_CHECK_ARG(total_length < ((int64_t)1 << 40), "resample_window: %sposition out of range", who);
    DMEL_CHECK_ARG(have_end <= total_length, "resample_window: %sthe buffer runs past the end of the signal", who);
    DMEL_CHECK_ARG(o0 + n_out <= (total_length * new_freq + orig_freq - 1) / orig_freq,
                   "resample_window: %soutputs past ceil(new_freq * total_length / orig_freq)", who);
  }
  const int64_t L = known ? total_length : ((int64_t)1 << 62);
  // every sample the outputs read must lie in the buffer or in the zero padding: output o reads
  // [(o / up) * down - width, (o / up) * down + width + down)
  const int64_t first = (o0 / new_freq) * orig_freq - width, last_end = ((o0 + n_out - 1) / new_freq) * orig_freq + width + orig_freq;
  const int64_t lo = std::max<int64_t>(first, 0), hi = std::min(last_end, L);
  DMEL_CHECK_ARG(lo >= hi || (s0 <= lo && hi <= have_end),
                 "resample_window: %soutputs [%lld, %lld) read samples [%lld, %lld), the buffer holds [%lld, %lld)", who, (long long)o0,
                 (long long)(o0 + n_out), (long long)lo, (long long)hi, (long long)s0, (long long)have_end);
  *L_out = L;
  return DMEL_OK;
}

extern "C" int dmel_resample_window_f32(const float* x, int64_t x_row_stride, int64_t n_samples, int64_t s0, float* y,
                                        const float* filter_bank_dev, int B, int64_t o0, int64_t n_out, int64_t total_length,
                                        int orig_freq, int new_freq, int width, void* stream) {
  DMEL_CHECK_ARG(x && y && filter_bank_dev, "resample_window: NULL argument");
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && orig_freq > 0 && new_freq > 0 && width >= 0, "resample_window: bad shape");
  DMEL_CHECK_ARG(x_row_stride >= n_samples, "resample_window: bad window");
  int64_t L;
  DMEL_TRY(resample_window_check(n_samples, s0, o0, n_out, total_length, orig_freq, new_freq, width, "", &L));
  return dmel::launch_resample_window(x, x_row_stride, s0, n_samples, y, filter_bank_dev, B, L, o0, n_out, orig_freq, new_freq, width,
                                      (hipStream_t)stream);
}

// ---- the same for B independent streams, each at its own rate (include/dmel_hip.h: dmel_resample_window_items_f32) ---------------
extern "C" int dmel_resample_window_items_f32(const float* x, int64_t x_row_stride, int64_t n_samples, const int64_t* s0,
                                              const int64_t* n_valid, float* y, int64_t y_row_stride, const int64_t* y_off,
                                              const float* bank_arena_dev, int64_t bank_arena_floats, const int64_t* rates, int n_rates,
                                              const int64_t* rate_index, int B, const int64_t* o0, const int64_t* n_out,
                                              const int64_t* total_length, int64_t* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(x && y && bank_arena_dev && s0 && n_valid && y_off && rates && rate_index && o0 && n_out && total_length && table_scratch,
                 "resample_window_items: NULL argument");
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && n_rates > 0 && n_rates <= 4096, "resample_window_items: bad shape");
  DMEL_CHECK_ARG(n_samples > 0 && x_row_stride >= n_samples && y_row_stride > 0 && bank_arena_floats > 0,
                 "resample_window_items: bad buffer width");
  std::vector<int64_t> tab((size_t)kResampleItemWords * B + (size_t)kResampleRateWords * n_rates, 0);   // an idle item keeps n_out = 0
  int64_t max_out = 0;
  int lds_floats = 0;
  double bytes = 0.0;
  for (int b = 0; b < B; ++b) {
    DMEL_CHECK_ARG(n_out[b] >= 0, "resample_window_items: item %d: negative output count", b);
    if (n_out[b] == 0) continue;
    DMEL_CHECK_ARG(rate_index[b] >= 0 && rate_index[b] < n_rates, "resample_window_items: item %d: rate %lld of %d", b,
                   (long long)rate_index[b], n_rates);
    const int64_t* r = rates + kResampleRateWords * rate_index[b];
    const int64_t bank_off = r[0], orig = r[1], nw = r[2], width = r[3];
    DMEL_CHECK_ARG(orig > 0 && nw > 0 && width >= 0 && orig < (1 << 20) && nw < (1 << 20) && width < (1 << 20),
                   "resample_window_items: item %d: bad rate %lld -> %lld, width %lld", b, (long long)orig, (long long)nw, (long long)width);
    const int64_t kw = 2 * width + orig;
    DMEL_CHECK_ARG(bank_off >= 0 && bank_off + nw * kw <= bank_arena_floats,
                   "resample_window_items: item %d: its bank [%lld, %lld) lies outside the arena of %lld floats", b, (long long)bank_off,
                   (long long)(bank_off + nw * kw), (long long)bank_arena_floats);
    DMEL_CHECK_ARG(n_valid[b] <= n_samples, "resample_window_items: item %d: %lld valid samples in a buffer of %lld", b,
                   (long long)n_valid[b], (long long)n_samples);
    DMEL_CHECK_ARG(y_off[b] >= 0 && y_off[b] + n_out[b] <= y_row_stride,
                   "resample_window_items: item %d: outputs [%lld, %lld) do not fit an output row of %lld", b, (long long)y_off[b],
                   (long long)(y_off[b] + n_out[b]), (long long)y_row_stride);
    char who[32];
    std::snprintf(who, sizeof(who), "item %d: ", b);
    int64_t L;
    DMEL_TRY(resample_window_check(n_valid[b], s0[b], o0[b], n_out[b], total_length[b], orig, nw, width, who, &L));
    int64_t* it = tab.data() + (size_t)kResampleItemWords * b;
    it[0] = s0[b]; it[1] = n_valid[b]; it[2] = o0[b]; it[3] = n_out[b]; it[4] = L; it[5] = y_off[b]; it[6] = rate_index[b];
    max_out = std::max(max_out, n_out[b]);
    if (nw * kw <= kResampleLdsFloats) lds_floats = std::max(lds_floats, (int)(nw * kw));
    bytes += 4.0 * ((double)n_valid[b] + (double)n_out[b]);
  }
  if (max_out == 0) return DMEL_OK;                   // every item idle
  std::memcpy(tab.data() + (size_t)kResampleItemWords * B, rates, (size_t)kResampleRateWords * n_rates * sizeof(int64_t));
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(int64_t), table_scratch, (hipStream_t)stream));
  return launch_resample_window_items(x, x_row_stride, y, y_row_stride, bank_arena_dev, B, table_scratch,
                                      table_scratch + (size_t)kResampleItemWords * B, max_out, lds_floats, bytes, (hipStream_t)stream);
}

// ---- B ragged convert-copies between 16-bit PCM, G.711 and fp32 in one launch (include/dmel_hip.h: dmel_pcm_convert_items) ---------
// bytes of one sample of a DMEL_SAMPLE_* format; 0: not a format (2 .. 7 are not assigned)
static int pcm_sample_bytes(int fmt) {
  return fmt == DMEL_SAMPLE_F32 ? 4 : fmt == DMEL_SAMPLE_S16 ? 2 : (fmt == DMEL_SAMPLE_ULAW || fmt == DMEL_SAMPLE_ALAW) ? 1 : 0;
}
extern "C" int dmel_pcm_convert_items(const void* const* src, const int32_t* src_fmt, void* const* dst, const int32_t* dst_fmt,
                                      const int64_t* n, int B, void* table_scratch, void* stream) {
  return dmel_pcm_convert_items_ch(src, src_fmt, nullptr, nullptr, dst, dst_fmt, nullptr, n, B, table_scratch, stream);
}
// the same with interleaved channels: n counts frames; src_ch / dst_ch / src_pick may be NULL (all 1, all 1, all -1)
extern "C" int dmel_pcm_convert_items_ch(const void* const* src, const int32_t* src_fmt, const int32_t* src_ch, const int32_t* src_pick,
                                         void* const* dst, const int32_t* dst_fmt, const int32_t* dst_ch, const int64_t* n, int B,
                                         void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(src && src_fmt && dst && dst_fmt && n && table_scratch, "pcm_convert_items: NULL argument");
  DMEL_CHECK_ARG(B >= 1 && B <= 65535, "pcm_convert_items: %d items, expected 1 .. 65535", B);
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 7) == 0, "pcm_convert_items: table_scratch is not 8-byte aligned");
  std::vector<int64_t> tab((size_t)kPcmItemWords * B, 0);           // an idle item keeps n = 0
  int64_t max_n = 0;
  double bytes = 0.0;
  for (int b = 0; b < B; ++b) {
    const int sf = src_fmt[b], df = dst_fmt[b];
    DMEL_CHECK_ARG(pcm_sample_bytes(sf) && pcm_sample_bytes(df),
                   "pcm_convert_items: item %d: sample formats %d -> %d, expected DMEL_SAMPLE_F32 (0), DMEL_SAMPLE_S16 (1), "
                   "DMEL_SAMPLE_ULAW (8) or DMEL_SAMPLE_ALAW (9)", b, sf, df);
    DMEL_CHECK_ARG(!(sf == DMEL_SAMPLE_S16 && df == DMEL_SAMPLE_S16), "pcm_convert_items: item %d: s16 -> s16 is not a conversion", b);
    DMEL_CHECK_ARG(sf == DMEL_SAMPLE_F32 || df == DMEL_SAMPLE_F32,
                   "pcm_convert_items: item %d: %d -> %d is not a conversion served here: mu-law and A-law convert from and to f32 only", b, sf,
                   df);
    const int sc = src_ch ? src_ch[b] : 1, dc = dst_ch ? dst_ch[b] : 1, pick = src_pick ? src_pick[b] : -1;
    DMEL_CHECK_ARG(sc >= 1 && sc <= DMEL_MAX_CHANNELS && dc >= 1 && dc <= DMEL_MAX_CHANNELS,
                   "pcm_convert_items: item %d: channel counts %d -> %d, expected 1 .. %d", b, sc, dc, DMEL_MAX_CHANNELS);
    DMEL_CHECK_ARG(sc == 1 || dc == 1, "pcm_convert_items: item %d: %d -> %d channels is not served: one side is mono", b, sc, dc);
    DMEL_CHECK_ARG(pick == -1 || (sc > 1 && pick >= 0 && pick < sc),
                   "pcm_convert_items: item %d: pick %d with %d source channels, expected -1 (the mean)%s", b, pick, sc,
                   sc > 1 ? " or a channel of the source" : "");
    const int ch = std::max(sc, dc);
    DMEL_CHECK_ARG(n[b] >= 0 && n[b] < ((int64_t)1 << 40) && n[b] * ch < ((int64_t)1 << 40),
                   "pcm_convert_items: item %d: sample count %lld out of range", b, (long long)n[b]);
    if (n[b] == 0) continue;
    DMEL_CHECK_ARG(src[b] && dst[b], "pcm_convert_items: item %d: NULL pointer with %lld samples", b, (long long)n[b]);
    const uintptr_t sa = (uintptr_t)src[b], da = (uintptr_t)dst[b];
    const int ss = pcm_sample_bytes(sf), ds = pcm_sample_bytes(df);   // a law pointer (1 byte) needs no alignment
    DMEL_CHECK_ARG(sa % ss == 0 && da % ds == 0, "pcm_convert_items: item %d: a pointer is not aligned to its sample size (%d -> %d bytes)", b,
                   ss, ds);
    int64_t* it = tab.data() + (size_t)kPcmItemWords * b;
    it[0] = (int64_t)sa; it[1] = (int64_t)da; it[2] = n[b];
    it[3] = sf | (df << 8) | ((sc - 1) << 16) | ((dc - 1) << 20) | ((pick + 1) << 24);   // a mono item: the word it always had
    max_n = std::max(max_n, n[b]);
    bytes += (double)n[b] * (ss * sc + ds * dc);
  }
  if (max_n == 0) return DMEL_OK;                     // every item idle
  hipStream_t s = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(int64_t), table_scratch, s));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per convert launch, so that a caller can tell
    // this launch from the other small ones of a step (dmel_prof_read("pcm_convert"))
    ProfScope ps("small", s, 0.0, bytes), count("pcm_convert", s, 0.0, 0.0);
    hipLaunchKernelGGL(pcm_convert_kernel, dim3((unsigned)((max_n + kPcmTile - 1) / kPcmTile), (unsigned)B), dim3(256), 0, s,
                       static_cast<const int64_t*>(table_scratch));
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- fork of streaming state between items of the same buffers (include/dmel_hip.h: dmel_stream_fork_items) --------------------------
// Row r of the table is (src, dst, lo, hi, first tile); a workgroup owns one tile of kForkTile columns of one channel row -- blockIdx.y
// runs over the (L + 1) C channel rows of hist, then the C of skip, the Ccond of cond and the Cout of mel -- of the row that owns tile
// blockIdx.x: the last one whose first tile is not behind it (an idle row owns no tile, so the row behind it starts where it does).
// The search and the row are uniform over the workgroup.  The 16-byte path is chosen per (row, channel): both addresses depend on the
// pitch, whole vectors on lo % 4 and hi % 4.  No LDS, no atomics; src and dst are different items, so no element is read and written.
constexpr int kForkWords = 5, kForkTile = 1024;
__global__ __launch_bounds__(256) void stream_fork_kernel(float* hist, float* skip, float* cond, float* mel, int L1, int N, int C, int Ccond,
                                                          int Cout, int64_t cap, const int32_t* __restrict__ tab, int R) {
  const int tile = blockIdx.x;
  int a = 0, b = R - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (tab[(size_t)mid * kForkWords + 4] <= tile) a = mid;
    else b = mid - 1;
  }
  const int32_t* row = tab + (size_t)a * kForkWords;
  const int src = __builtin_amdgcn_readfirstlane(row[0]), dst = __builtin_amdgcn_readfirstlane(row[1]);
  const int lo = __builtin_amdgcn_readfirstlane(row[2]), hi = __builtin_amdgcn_readfirstlane(row[3]);
  const int first = lo + (tile - __builtin_amdgcn_readfirstlane(row[4])) * kForkTile;
  if (first < lo || first >= hi) return;
  int j = blockIdx.y;
  float* base;
  int64_t so, dn;
  if (j < L1 * C) {
    const int lev = j / C, c = j % C;
    base = hist; so = (((int64_t)lev * N + src) * C + c) * cap; dn = (((int64_t)lev * N + dst) * C + c) * cap;
  } else if ((j -= L1 * C) < C) {
    base = skip; so = ((int64_t)src * C + j) * cap; dn = ((int64_t)dst * C + j) * cap;
  } else if ((j -= C) < Ccond) {
    base = cond; so = ((int64_t)src * Ccond + j) * cap; dn = ((int64_t)dst * Ccond + j) * cap;
  } else {
    j -= Ccond;
    if (j >= Cout) return;
    base = mel; so = ((int64_t)src * Cout + j) * cap; dn = ((int64_t)dst * Cout + j) * cap;
  }
  const float* s = base + so;
  float* d = base + dn;
  const int end = min(hi, first + kForkTile);
  const bool vec = ((lo | hi) & 3) == 0 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
  if (vec) {
    const int t = first + 4 * (int)threadIdx.x;
    if (t < end) *reinterpret_cast<float4*>(d + t) = *reinterpret_cast<const float4*>(s + t);
  } else {
    for (int t = first + (int)threadIdx.x; t < end; t += 256) d[t] = s[t];
  }
}

}  // namespace dmel

extern "C" int dmel_stream_fork_items(float* hist, float* skip, float* cond, float* mel, int L, int N, int C, int Ccond, int Cout, int64_t cap,
                                      int R, const int64_t* src, const int64_t* dst, const int64_t* lo, const int64_t* hi,
                                      void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(hist && skip && mel && src && dst && lo && hi && table_scratch, "stream_fork_items: NULL argument");
  DMEL_CHECK_ARG((Ccond != 0) == (cond != nullptr), "stream_fork_items: the condition tensor is given exactly when Ccond is not 0");
  DMEL_CHECK_ARG(L >= 0 && N > 0 && N <= 65535 && C > 0 && Ccond >= 0 && Cout > 0 && cap > 0 && cap < ((int64_t)1 << 30) && R > 0 && R <= 65535,
                 "stream_fork_items: bad shape");
  const int64_t chan_rows = (int64_t)(L + 2) * C + Ccond + Cout;
  DMEL_CHECK_ARG(chan_rows <= 65535, "stream_fork_items: %lld channel rows per item exceed 65535", (long long)chan_rows);
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 3) == 0, "stream_fork_items: table_scratch is not 4-byte aligned");
  std::vector<int32_t> tab((size_t)kForkWords * R);
  std::vector<int> role(N, -1);                       // the row that writes the item; -2: some row reads it
  int64_t tiles = 0, cols = 0;
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(src[r] >= 0 && src[r] < N && dst[r] >= 0 && dst[r] < N, "stream_fork_items: row %d: items %lld -> %lld outside [0, %d)", r,
                   (long long)src[r], (long long)dst[r], N);
    DMEL_CHECK_ARG(src[r] != dst[r], "stream_fork_items: row %d: item %lld is forked into itself", r, (long long)src[r]);
    DMEL_CHECK_ARG(lo[r] >= 0 && lo[r] <= hi[r] && hi[r] <= cap, "stream_fork_items: row %d: window [%lld, %lld) outside [0, %lld]", r,
                   (long long)lo[r], (long long)hi[r], (long long)cap);
  }
  for (int r = 0; r < R; ++r) role[src[r]] = -2;
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(role[dst[r]] == -1, "stream_fork_items: row %d: its destination, item %lld, is %s", r, (long long)dst[r],
                   role[dst[r]] == -2 ? "the source of a row" : "the destination of another row as well");
    role[dst[r]] = r;
    int32_t* it = tab.data() + (size_t)kForkWords * r;
    it[0] = (int32_t)src[r]; it[1] = (int32_t)dst[r]; it[2] = (int32_t)lo[r]; it[3] = (int32_t)hi[r]; it[4] = (int32_t)tiles;
    tiles += (hi[r] - lo[r] + kForkTile - 1) / kForkTile;
    cols += hi[r] - lo[r];
  }
  if (tiles == 0) return DMEL_OK;                     // every row idle
  hipStream_t s = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(int32_t), table_scratch, s));
  {
    ProfScope ps("small", s, 0.0, 8.0 * (double)chan_rows * (double)cols), count("stream_fork", s, 0.0, 0.0);
    hipLaunchKernelGGL(stream_fork_kernel, dim3((unsigned)tiles, (unsigned)chan_rows), dim3(256), 0, s, hist, skip, cond, mel, L + 1, N, C, Ccond,
                       Cout, cap, static_cast<const int32_t*>(table_scratch), R);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- cross-fade of provisional audio pieces (include/dmel_hip.h: dmel_crossfade_items) -------------------------------------------------
// Row r of the table is (blend, tail, save, w, F), five int64; a workgroup owns kFadeTile elements of row blockIdx.y, a lane four
// consecutive ones.  Per element: old = tail[i]; blend[i] = old + w[i] * (blend[i] - old) where blend is set; tail[i] = save[i] where save
// is set.  The three operations are rounded one by one (fp contract(off) in fade_blend: nothing is fused into an fma), which is what
// the fp32 torch expression gives on the host.  The row is uniform over the workgroup; its 16-byte path is taken when F is a
// multiple of 4 and every pointer of the row is 16-byte aligned.  No LDS, no atomics; a lane reads its tail before it writes it, and
// the blend and save regions of a row do not overlap (the caller's contract), so no element is read after another lane wrote it.
constexpr int kFadeWords = 5, kFadeTile = 1024;
__device__ __forceinline__ float fade_blend(float old, float w, float now) {
  // hipcc contracts by default, and through __fmul_rn / __fadd_rn as well (they are plain operators here): the pragma is what keeps
  // the product rounded before the sum
#pragma clang fp contract(off)
  const float d = now - old;
  const float p = w * d;
  return old + p;
}
__global__ __launch_bounds__(256) void crossfade_kernel(const int64_t* __restrict__ tab) {
  const int64_t* row = tab + (size_t)blockIdx.y * kFadeWords;
  float* blend = reinterpret_cast<float*>(row[0]);
  float* tail = reinterpret_cast<float*>(row[1]);
  const float* save = reinterpret_cast<const float*>(row[2]);
  const float* w = reinterpret_cast<const float*>(row[3]);
  const int F = (int)row[4];
  const int i = (int)blockIdx.x * kFadeTile + 4 * (int)threadIdx.x;
  if (i >= F) return;
  const bool vec = (F & 3) == 0 && ((row[0] | row[1] | row[2] | row[3]) & 15) == 0;   // a NULL pointer is aligned
  if (vec) {
    const float4 old = *reinterpret_cast<const float4*>(tail + i);
    if (blend) {
      const float4 x = *reinterpret_cast<const float4*>(blend + i), ww = *reinterpret_cast<const float4*>(w + i);
      *reinterpret_cast<float4*>(blend + i) = make_float4(fade_blend(old.x, ww.x, x.x), fade_blend(old.y, ww.y, x.y),
                                                          fade_blend(old.z, ww.z, x.z), fade_blend(old.w, ww.w, x.w));
    }
    if (save) *reinterpret_cast<float4*>(tail + i) = *reinterpret_cast<const float4*>(save + i);
  } else {
    const int end = min(F, i + 4);
    for (int t = i; t < end; ++t) {
      const float old = tail[t];
      if (blend) blend[t] = fade_blend(old, w[t], blend[t]);
      if (save) tail[t] = save[t];
    }
  }
}

}  // namespace dmel

extern "C" int dmel_crossfade_items(float* const* blend, float* const* tail, const float* const* save, const float* const* w,
                                    const int64_t* F, int R, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(blend && tail && save && w && F && table_scratch, "crossfade_items: NULL argument");
  DMEL_CHECK_ARG(R >= 1 && R <= 65535, "crossfade_items: %d rows, expected 1 .. 65535", R);
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 7) == 0, "crossfade_items: table_scratch is not 8-byte aligned");
  std::vector<int64_t> tab((size_t)kFadeWords * R);
  int64_t max_f = 0;
  double bytes = 0.0;
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(F[r] >= 1 && F[r] <= 4096, "crossfade_items: row %d: a fade of %lld samples, expected 1 .. 4096", r, (long long)F[r]);
    DMEL_CHECK_ARG(tail[r] && w[r], "crossfade_items: row %d: NULL tail or weights", r);
    DMEL_CHECK_ARG(blend[r] || save[r], "crossfade_items: row %d: neither blend nor save: nothing to do", r);
    DMEL_CHECK_ARG((((uintptr_t)blend[r] | (uintptr_t)tail[r] | (uintptr_t)save[r] | (uintptr_t)w[r]) & 3) == 0,
                   "crossfade_items: row %d: a pointer is not 4-byte aligned", r);
    int64_t* it = tab.data() + (size_t)kFadeWords * r;
    it[0] = (int64_t)(uintptr_t)blend[r]; it[1] = (int64_t)(uintptr_t)tail[r]; it[2] = (int64_t)(uintptr_t)save[r];
    it[3] = (int64_t)(uintptr_t)w[r]; it[4] = F[r];
    max_f = std::max(max_f, F[r]);
    bytes += 4.0 * (double)F[r] * ((blend[r] ? 3 : 0) + (save[r] ? 2 : 0) + 1);
  }
  hipStream_t s = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(int64_t), table_scratch, s));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per cross-fade launch (dmel_prof_read("crossfade"))
    ProfScope ps("small", s, 0.0, bytes), count("crossfade", s, 0.0, 0.0);
    hipLaunchKernelGGL(crossfade_kernel, dim3((unsigned)((max_f + kFadeTile - 1) / kFadeTile), (unsigned)R), dim3(256), 0, s,
                       static_cast<const int64_t*>(table_scratch));
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- ragged 2-D copies of 4-byte words: streaming state into and out of a snapshot (include/dmel_hip.h: dmel_stream_pack_items) ------
// Row r of the table is (src, dst, rows, cols, src pitch, dst pitch, first tile, column tiles), eight int64; a workgroup owns one tile of
// kPackRows rows by kPackCols columns of the descriptor that owns tile blockIdx.x: the last one whose first tile is not behind it (an
// idle descriptor owns no tile, so the one behind it starts where it does).  The search and the row are uniform over the workgroup.
// A wave takes one row of the tile at a time, rows w and w + 4: in the 16-byte path a lane moves one uint4, 1 KiB per wave and
// instruction, and the lane that meets the end of the row moves its last cols % 4 words one by one; in the word path a lane moves the
// words lane, lane + 64, ... of the row.  Words are uint32 on both paths: no float is ever formed.  No LDS, no atomics.
constexpr int kPackWords = 8, kPackRows = 8, kPackCols = 256;
__global__ __launch_bounds__(256) void stream_pack_kernel(const int64_t* __restrict__ tab, int R) {
  const int64_t tile = blockIdx.x;
  int a = 0, b = R - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (tab[(size_t)mid * kPackWords + 6] <= tile) a = mid;
    else b = mid - 1;
  }
  const int64_t* row = tab + (size_t)a * kPackWords;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(row[0]);
  uint32_t* dst = reinterpret_cast<uint32_t*>(row[1]);
  const int64_t rows = row[2], cols = row[3], sp = row[4], dp = row[5], local = tile - row[6], ct = row[7];
  if (ct <= 0 || local < 0) return;
  const int64_t r0 = (local / ct) * kPackRows, c0 = (local % ct) * kPackCols;
  if (r0 >= rows || c0 >= cols) return;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const bool vec = ((row[0] | row[1]) & 15) == 0 && (rows == 1 || ((sp | dp) & 3) == 0);
  for (int k = wave; k < kPackRows; k += 4) {
    const int64_t i = r0 + k;
    if (i >= rows) break;
    const uint32_t* s = src + i * sp;
    uint32_t* d = dst + i * dp;
    if (vec) {
      const int64_t c = c0 + 4 * lane;
      if (c + 4 <= cols) {
        *reinterpret_cast<uint4*>(d + c) = *reinterpret_cast<const uint4*>(s + c);
      } else {
        for (int64_t t = c; t < cols; ++t) d[t] = s[t];
      }
    } else {
      const int64_t end = c0 + kPackCols < cols ? c0 + kPackCols : cols;
      for (int64_t t = c0 + lane; t < end; t += 64) d[t] = s[t];
    }
  }
}

}  // namespace dmel

extern "C" int dmel_stream_pack_items(const void* const* src, void* const* dst, const int64_t* rows, const int64_t* cols,
                                      const int64_t* src_pitch, const int64_t* dst_pitch, int R, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(src && dst && rows && cols && src_pitch && dst_pitch && table_scratch, "stream_pack_items: NULL argument");
  DMEL_CHECK_ARG(R >= 1 && R <= 65535, "stream_pack_items: %d rows, expected 1 .. 65535", R);
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 7) == 0, "stream_pack_items: table_scratch is not 8-byte aligned");
  std::vector<int64_t> tab((size_t)kPackWords * R);
  const int64_t limit = (int64_t)1 << 40;
  int64_t tiles = 0;
  double words = 0.0;
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(rows[r] >= 0 && cols[r] >= 0, "stream_pack_items: row %d: %lld rows of %lld words: a negative count", r, (long long)rows[r],
                   (long long)cols[r]);
    int64_t* it = tab.data() + (size_t)kPackWords * r;
    it[6] = tiles;
    if (rows[r] == 0 || cols[r] == 0) continue;       // idle: its pointers and pitches are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(src[r] && dst[r], "stream_pack_items: row %d: NULL source or destination", r);
    DMEL_CHECK_ARG((((uintptr_t)src[r] | (uintptr_t)dst[r]) & 3) == 0, "stream_pack_items: row %d: a pointer is not 4-byte aligned", r);
    DMEL_CHECK_ARG(rows[r] < limit && cols[r] < limit, "stream_pack_items: row %d: %lld rows of %lld words exceed 2^40", r, (long long)rows[r],
                   (long long)cols[r]);
    if (rows[r] > 1) {
      DMEL_CHECK_ARG(src_pitch[r] >= cols[r] && dst_pitch[r] >= cols[r],
                     "stream_pack_items: row %d: pitches %lld and %lld are below its %lld words per row", r, (long long)src_pitch[r],
                     (long long)dst_pitch[r], (long long)cols[r]);
      const int64_t top = (limit - 1) / rows[r];       // rows * pitch < 2^40 without forming a product that can overflow int64
      DMEL_CHECK_ARG(src_pitch[r] <= top && dst_pitch[r] <= top,
                     "stream_pack_items: row %d: %lld rows at pitches %lld and %lld exceed 2^40 words", r, (long long)rows[r],
                     (long long)src_pitch[r], (long long)dst_pitch[r]);
    }
    const int64_t ct = (cols[r] + kPackCols - 1) / kPackCols, rt = (rows[r] + kPackRows - 1) / kPackRows;
    it[0] = (int64_t)(uintptr_t)src[r]; it[1] = (int64_t)(uintptr_t)dst[r]; it[2] = rows[r]; it[3] = cols[r];
    it[4] = rows[r] > 1 ? src_pitch[r] : 0; it[5] = rows[r] > 1 ? dst_pitch[r] : 0; it[7] = ct;
    tiles += ct * rt;
    DMEL_CHECK_ARG(tiles <= 0x7fffffff, "stream_pack_items: row %d: more than 2^31 - 1 tiles", r);
    words += (double)rows[r] * (double)cols[r];
  }
  if (tiles == 0) return DMEL_OK;                     // every row idle
  hipStream_t s = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(int64_t), table_scratch, s));
  {
    ProfScope ps("small", s, 0.0, 8.0 * words), count("stream_pack", s, 0.0, 0.0);
    hipLaunchKernelGGL(stream_pack_kernel, dim3((unsigned)tiles), dim3(256), 0, s, static_cast<const int64_t*>(table_scratch), R);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- voice activity and end of turn on log-mel frames (include/dmel_hip.h: dmel_voice_items; the rule: utils/voice.py) ---------------
// Row s of the table is (frames, threshold, min_level, fall, rise, rise_speech, band_lo, band_hi, min_bands, attack, release, 0), twelve
// 4-byte words; workgroup s is ONE wave and owns slot s, lane l the bands l and l + 64, whose floors stay in registers from the first
// frame of the launch to the last.  The slot's tile passes through LDS in chunks of kVoiceChunk frames: the wave reads 64 consecutive
// frames of one band per instruction (256 contiguous bytes) and writes them as one row of pitch kVoiceChunk + 1 words, so that the
// frame loop's column reads (lane l at word l * 65 + t) hit 32 different banks in each half of the wave.  The frame loop is
// sequential: the coefficient of frame f depends on the state after frame f - 1.  The band count is two ballots; every lane then
// runs the same state machine on the same integers, so nothing inside the frame loop waits for another lane.  Lane t keeps the two
// output bytes of frame t of the chunk and stores them behind the loop: 64 consecutive bytes per row.  The floor update is three
// separately rounded operations (fp contract(off) in voice_floor, as fade_blend above): what the fp32 host expression gives.  Plain
// stores, no atomics.
constexpr int kVoiceWords = 12, kVoiceChunk = 64, kVoiceMaxMels = 128, kVoicePitch = kVoiceChunk + 1;
__device__ __forceinline__ float voice_floor(float fl, float L, bool first, float fall, float up, float min_level) {
#pragma clang fp contract(off)
  float v = L;
  if (!first) {
    const float c = L < fl ? fall : up;
    const float d = L - fl;
    const float p = c * d;
    v = fl + p;
  }
  return v < min_level ? min_level : v;
}
__global__ __launch_bounds__(64) void voice_kernel(const float* __restrict__ mel, int64_t item_stride, int64_t band_stride, int n_mels,
                                                   const uint32_t* __restrict__ tab, uint32_t* __restrict__ state,
                                                   uint8_t* __restrict__ flags, uint8_t* __restrict__ counts, int64_t out_pitch) {
  __shared__ float tile[kVoiceMaxMels * kVoicePitch];
  const int s = blockIdx.x, lane = threadIdx.x;
  const uint32_t* row = tab + (size_t)s * kVoiceWords;
  const int n = (int)row[0];
  if (n <= 0) return;                                   // idle (uniform: in front of the first barrier)
  const float thr = __uint_as_float(row[1]), min_level = __uint_as_float(row[2]), fall = __uint_as_float(row[3]);
  const float rise = __uint_as_float(row[4]), rise_speech = __uint_as_float(row[5]);
  const int lo = (int)row[6], hi = (int)row[7], min_bands = (int)row[8], attack = (int)row[9], release = (int)row[10];
  uint32_t* srow = state + (size_t)s * (n_mels + 8);
  const int32_t* ints = reinterpret_cast<const int32_t*>(srow + n_mels);
  const int b0 = lane, b1 = lane + 64;
  const bool have0 = b0 < n_mels, have1 = b1 < n_mels;
  const bool win0 = have0 && b0 >= lo && b0 < hi, win1 = have1 && b1 >= lo && b1 < hi;
  float fl0 = have0 ? __uint_as_float(srow[b0]) : 0.0f, fl1 = have1 ? __uint_as_float(srow[b1]) : 0.0f;
  int st = ints[0], run = ints[1], seen = ints[2], start = ints[3], end = ints[4], starts = ints[5], act_frames = ints[6];
  if (seen == 0) start = end = -1;                      // a zeroed row: the fresh session
  const float* src = mel + (int64_t)s * item_stride;
  for (int f0 = 0; f0 < n; f0 += kVoiceChunk) {
    const int m = min(kVoiceChunk, n - f0);
    if (lane < m)
      for (int b = 0; b < n_mels; ++b) tile[b * kVoicePitch + lane] = src[(int64_t)b * band_stride + f0 + lane];
    __syncthreads();
    uint32_t my_flag = 0, my_count = 0;
    for (int t = 0; t < m; ++t) {
      const float L0 = have0 ? tile[b0 * kVoicePitch + t] : 0.0f, L1 = have1 ? tile[b1 * kVoicePitch + t] : 0.0f;
      const float up = st == 0 ? rise : rise_speech;
      fl0 = voice_floor(fl0, L0, seen == 0, fall, up, min_level);
      fl1 = voice_floor(fl1, L1, seen == 0, fall, up, min_level);
      const bool e0 = win0 && L0 > min_level && (L0 - fl0) > thr, e1 = win1 && L1 > min_level && (L1 - fl1) > thr;
      const int count = __popcll(__ballot(e0)) + __popcll(__ballot(e1));
      const int active = count >= min_bands ? 1 : 0;
      run = (active != (st == 1 ? 1 : 0)) ? run + 1 : 0;
      if (st == 0 && run >= attack) {
        st = 1; start = seen - run + 1; starts += 1; run = 0;
      } else if (st == 1 && run >= release) {
        st = 0; end = seen - run + 1; run = 0;
      }
      seen += 1;
      act_frames += active;
      if (lane == t) { my_flag = (uint32_t)(active | st << 1); my_count = (uint32_t)count; }
    }
    if (lane < m) {
      if (flags) flags[(int64_t)s * out_pitch + f0 + lane] = (uint8_t)my_flag;
      if (counts) counts[(int64_t)s * out_pitch + f0 + lane] = (uint8_t)my_count;
    }
    __syncthreads();                                    // the next chunk overwrites the tile
  }
  if (have0) srow[b0] = __float_as_uint(fl0);
  if (have1) srow[b1] = __float_as_uint(fl1);
  if (lane < 8) {
    const int v = lane == 0 ? st : lane == 1 ? run : lane == 2 ? seen : lane == 3 ? start : lane == 4 ? end : lane == 5 ? starts
                : lane == 6 ? act_frames : 0;
    srow[n_mels + lane] = (uint32_t)v;
  }
}

}  // namespace dmel

extern "C" int dmel_voice_items(const float* mel, int64_t item_stride, int64_t band_stride, int n_mels, int S, const int64_t* n_frames,
                                const float* fparams, const int32_t* iparams, void* state, uint8_t* flags, uint8_t* counts,
                                int64_t out_pitch, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(mel && n_frames && fparams && iparams && state && table_scratch, "voice_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "voice_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG(n_mels >= 1 && n_mels <= kVoiceMaxMels, "voice_items: %d mel bands, expected 1 .. %d", n_mels, kVoiceMaxMels);
  DMEL_CHECK_ARG((((uintptr_t)mel | (uintptr_t)state | (uintptr_t)table_scratch) & 3) == 0,
                 "voice_items: mel, state or table_scratch is not 4-byte aligned");
  DMEL_CHECK_ARG(item_stride >= 0 && band_stride >= 0, "voice_items: negative strides (%lld, %lld)", (long long)item_stride,
                 (long long)band_stride);
  std::vector<uint32_t> tab((size_t)kVoiceWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_frames[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x7fffffff, "voice_items: item %d: %lld frames, expected 0 .. 2^31 - 1", s, (long long)n);
    if (n == 0) continue;                               // idle: its parameters are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(out_pitch >= n, "voice_items: item %d: %lld frames exceed the output pitch %lld", s, (long long)n, (long long)out_pitch);
    const float* fp = fparams + (size_t)5 * s;
    const int32_t* ip = iparams + (size_t)5 * s;
    for (int k = 0; k < 5; ++k) DMEL_CHECK_ARG(std::isfinite(fp[k]), "voice_items: item %d: float parameter %d is not finite", s, k);
    DMEL_CHECK_ARG(fp[0] > 0.0f, "voice_items: item %d: threshold %g, expected > 0", s, (double)fp[0]);
    DMEL_CHECK_ARG(fp[2] > 0.0f && fp[2] <= 1.0f && fp[3] > 0.0f && fp[3] <= 1.0f,
                   "voice_items: item %d: fall %g or rise %g outside (0, 1]", s, (double)fp[2], (double)fp[3]);
    DMEL_CHECK_ARG(fp[4] >= 0.0f && fp[4] <= 1.0f, "voice_items: item %d: rise_speech %g outside [0, 1]", s, (double)fp[4]);
    DMEL_CHECK_ARG(ip[0] >= 0 && ip[0] < ip[1] && ip[1] <= n_mels, "voice_items: item %d: bands [%d, %d) are not a window of the %d bands",
                   s, ip[0], ip[1], n_mels);
    DMEL_CHECK_ARG(ip[2] >= 1 && ip[2] <= ip[1] - ip[0], "voice_items: item %d: min_bands %d outside [1, %d]", s, ip[2], ip[1] - ip[0]);
    DMEL_CHECK_ARG(ip[3] >= 1 && ip[3] <= (1 << 20) && ip[4] >= 1 && ip[4] <= (1 << 20),
                   "voice_items: item %d: attack_frames %d or release_frames %d outside [1, 2^20]", s, ip[3], ip[4]);
    uint32_t* it = tab.data() + (size_t)kVoiceWords * s;
    it[0] = (uint32_t)n;
    std::memcpy(it + 1, fp, 5 * sizeof(float));
    std::memcpy(it + 6, ip, 5 * sizeof(int32_t));
    ++live;
    bytes += (double)n * (4.0 * n_mels + (flags ? 1 : 0) + (counts ? 1 : 0)) + 8.0 * (n_mels + 8);
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per detector launch (dmel_prof_read("voice"))
    ProfScope ps("small", st, 0.0, bytes), count("voice", st, 0.0, 0.0);
    hipLaunchKernelGGL(voice_kernel, dim3((unsigned)S), dim3(64), 0, st, mel, item_stride, band_stride, n_mels,
                       static_cast<const uint32_t*>(table_scratch), static_cast<uint32_t*>(state), flags, counts, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- DTMF keys on codec-rate samples (include/dmel_hip.h: dmel_dtmf_items; the rule and the state row: utils/dtmf.py) ----------------
// Row s of the table is (first, n_new, N, c_0 .. c_7, emin, rel, max_col_over_row, max_row_over_col, g, hits, misses, 0, 0), twenty
// 4-byte words; workgroup s owns slot s.  The blocks a launch touches are independent but for the first, which continues the carried
// s1 / s2 / e of the state row and has consumed `fill` samples already: block j of the launch holds positions [j N, (j + 1) N) of the
// stream that began `fill` samples in front of column `first`, of which [fill, fill + n_new) exist.  So the parallel axis is
// (block, filter): nine lanes serve a block -- eight Goertzel recursions and the energy --, a wave seven blocks (lane 63 rests), the
// four waves of the workgroup 28 blocks per pass.  The samples of a pass go through LDS in chunks of kDtmfChunk per block: row j of
// the tile is block j's samples [t0, t0 + 64), read from global memory along the row (plain 4-byte loads: `first` is any column) and
// zero where the stream has no sample; the pitch of 65 words puts the seven rows a wave reads in one step on seven banks, and the
// nine lanes of a block read one word, a broadcast.  Whole blocks leave their eight powers and their energy in LDS, one thread per
// block decides, and every thread then runs the same state machine over the pass's decisions in block order (integers only, as
// voice_kernel does); thread j keeps the two output bytes of block j, thread 0 writes the events.  The trailing partial block's
// s1 / s2 / e go back to the row.  The recursion, the power, the energy and the compares are separately rounded operations
// (fp contract(off), as voice_floor above): what the fp32 host expression gives.  Plain stores, no atomics.
constexpr int kDtmfWords = 20, kDtmfChunk = 64, kDtmfPitch = kDtmfChunk + 1, kDtmfPass = 28, kDtmfState = 128, kDtmfRing = 32;
constexpr int kDtmfMinBlock = 32, kDtmfMaxBlock = 4096;
__device__ __forceinline__ void dtmf_step(float x, float c, float& s1, float& s2) {
#pragma clang fp contract(off)
  const float p = c * s1;
  const float q = p - s2;
  const float s0 = x + q;
  s2 = s1;
  s1 = s0;
}
__device__ __forceinline__ float dtmf_energy(float e, float x) {
#pragma clang fp contract(off)
  const float sq = x * x;
  return e + sq;
}
__device__ __forceinline__ float dtmf_power(float c, float s1, float s2) {
#pragma clang fp contract(off)
  const float a = s1 * s1, b = s2 * s2, m = s1 * s2;
  const float sum = a + b, cm = c * m;
  return sum - cm;
}
// key + 1 of a whole block, or 0: P[0 .. 3] the row powers, P[4 .. 7] the column powers, P[8] the energy
__device__ __forceinline__ int dtmf_decide(const float* P, float emin, float rel, float mcr, float mrc, float g) {
#pragma clang fp contract(off)
  int r = 0, c = 0;
  for (int j = 1; j < 4; ++j) {
    if (P[j] > P[r]) r = j;                             // the lowest index wins a tie
    if (P[4 + j] > P[4 + c]) c = j;
  }
  const float Pr = P[r], Pc = P[4 + c], E = P[8];
  bool ok = E > emin;
  for (int j = 0; j < 4; ++j) {
    const float tr = rel * P[j], tc = rel * P[4 + j];
    if (j != r) ok = ok && Pr > tr;
    if (j != c) ok = ok && Pc > tc;
  }
  const float lim_c = mcr * Pr, lim_r = mrc * Pc, both = Pr + Pc, need = g * E;
  ok = ok && Pc <= lim_c && Pr <= lim_r && both > need;
  return ok ? 4 * r + c + 1 : 0;
}
__global__ __launch_bounds__(256) void dtmf_kernel(const float* __restrict__ samples, int64_t row_stride, const uint32_t* __restrict__ tab,
                                                   uint32_t* __restrict__ state, uint8_t* __restrict__ decided,
                                                   uint8_t* __restrict__ pressed, int64_t out_pitch) {
  __shared__ float tile[kDtmfPass * kDtmfPitch];
  __shared__ float pw[kDtmfPass * 9];
  __shared__ int dec[kDtmfPass];
  const int s = blockIdx.x, tid = threadIdx.x;
  const uint32_t* row = tab + (size_t)s * kDtmfWords;
  const int64_t n_new = (int64_t)(int32_t)row[1];
  if (n_new <= 0) return;                               // idle (uniform: in front of the first barrier)
  const int64_t first = (int64_t)(int32_t)row[0];
  const int N = (int)row[2];
  const int lane = tid & 63, jb = lane / 9, k = lane - 9 * jb, jw = (tid >> 6) * 7 + jb;      // block jw of the pass, filter k (8: energy)
  const float coef = k < 8 ? __uint_as_float(row[3 + k]) : 0.0f;
  const float emin = __uint_as_float(row[11]), rel = __uint_as_float(row[12]), mcr = __uint_as_float(row[13]);
  const float mrc = __uint_as_float(row[14]), g = __uint_as_float(row[15]);
  const int hits = (int)row[16], misses = (int)row[17];
  uint32_t* srow = state + (size_t)s * kDtmfState;
  const int32_t* ints = reinterpret_cast<const int32_t*>(srow);
  int fill = ints[17];
  if ((unsigned)fill >= (unsigned)N) fill = 0;          // no row the rule wrote; keeps every index below inside the launch's columns
  int blocks = ints[18], down = ints[19], cand = ints[20], run = ints[21], miss = ints[22], events = ints[23];
  const int64_t end = fill + n_new;                     // positions [fill, end) exist
  const int64_t nblk = (end + N - 1) / N, done = end / N;
  const float* src = samples + (int64_t)s * row_stride + first - fill;       // position p is src[p]; only [fill, end) is read
  uint8_t* dout = decided + (int64_t)s * out_pitch;
  uint8_t* pout = pressed + (int64_t)s * out_pitch;
  for (int64_t b0 = 0; b0 < nblk; b0 += kDtmfPass) {
    const int nb = (int)min((int64_t)kDtmfPass, nblk - b0);
    const int nd = (int)max((int64_t)0, min((int64_t)nb, done - b0));          // the whole blocks of the pass
    const int64_t B = b0 + jw;
    const bool mine = jb < 7 && jw < nb;
    const int i0 = (mine && B == 0) ? fill : 0;
    const int i1 = mine ? (int)min((int64_t)N, end - B * N) : 0;
    float s1 = 0.0f, s2 = 0.0f;                         // the energy lane keeps e in s1
    if (mine && B == 0) {
      if (k < 8) { s1 = __uint_as_float(srow[k]); s2 = __uint_as_float(srow[8 + k]); }
      else s1 = __uint_as_float(srow[16]);
    }
    // the samples the pass's blocks still need: [t_lo, t_hi) of each (one block alone may begin and end inside itself)
    const int t_lo = (nb == 1 && b0 == 0) ? fill : 0;
    const int t_hi = nb > 1 ? N : (int)min((int64_t)N, end - b0 * N);
    for (int t0 = t_lo - t_lo % kDtmfChunk; t0 < t_hi; t0 += kDtmfChunk) {
      for (int idx = tid; idx < nb * kDtmfChunk; idx += 256) {
        const int r = idx / kDtmfChunk, cidx = idx % kDtmfChunk, i = t0 + cidx;
        const int64_t p = (b0 + r) * N + i;
        tile[r * kDtmfPitch + cidx] = (i < N && p >= fill && p < end) ? src[p] : 0.0f;
      }
      __syncthreads();
      if (mine) {
        const float* xs = tile + jw * kDtmfPitch;
        const int a = max(i0, t0) - t0, z = min(i1, t0 + kDtmfChunk) - t0;
        if (k < 8) {
          for (int t = a; t < z; ++t) dtmf_step(xs[t], coef, s1, s2);
        } else {
          for (int t = a; t < z; ++t) s1 = dtmf_energy(s1, xs[t]);
        }
      }
      __syncthreads();                                  // the next chunk overwrites the tile
    }
    if (mine) {
      if (i1 == N) {
        pw[jw * 9 + k] = k < 8 ? dtmf_power(coef, s1, s2) : s1;
      } else {                                          // the open block: its carry goes back to the row
        srow[k < 8 ? k : 16] = __float_as_uint(s1);
        if (k < 8) srow[8 + k] = __float_as_uint(s2);
      }
    }
    __syncthreads();
    if (tid < nd) dec[tid] = dtmf_decide(pw + tid * 9, emin, rel, mcr, mrc, g);
    __syncthreads();
    uint32_t my_dec = 0, my_down = 0;
    for (int j = 0; j < nd; ++j) {
      const int d = dec[j];
      if (down == 0) {
        if (d == 0) { cand = 0; run = 0; }
        else if (d == cand) run += 1;
        else { cand = d; run = 1; }
        if (cand != 0 && run >= hits) {
          down = cand; miss = 0;
          if (tid == 0) {
            uint32_t* ev = srow + 32 + 3 * ((uint32_t)events % kDtmfRing);
            ev[0] = (uint32_t)down; ev[1] = (uint32_t)(blocks - run + 1); ev[2] = 0xffffffffu;
          }
          events += 1;
        }
      } else if (d == down) {
        miss = 0;
      } else {
        miss += 1;
        if (miss >= misses) {
          if (tid == 0) srow[32 + 3 * ((uint32_t)(events - 1) % kDtmfRing) + 2] = (uint32_t)(blocks - miss + 1);
          down = 0; cand = 0; run = 0; miss = 0;
        }
      }
      blocks += 1;
      if (tid == j) { my_dec = (uint32_t)d; my_down = (uint32_t)down; }
    }
    if (tid < nd) {
      dout[b0 + tid] = (uint8_t)my_dec;
      pout[b0 + tid] = (uint8_t)my_down;
    }
  }
  const int left = (int)(end - done * N);               // the open block's samples
  if (left == 0 && tid < 17) srow[tid] = 0u;            // a whole last block: the carry is the fresh one
  if (tid == 0) {
    srow[17] = (uint32_t)left; srow[18] = (uint32_t)blocks; srow[19] = (uint32_t)down; srow[20] = (uint32_t)cand;
    srow[21] = (uint32_t)run; srow[22] = (uint32_t)miss; srow[23] = (uint32_t)events;
  }
}

}  // namespace dmel

extern "C" int dmel_dtmf_items(const float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new,
                               const int32_t* N, const float* coef, const float* fparams, const int32_t* iparams, void* state,
                               uint8_t* decided, uint8_t* pressed, int64_t out_pitch, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(samples && first && n_new && N && coef && fparams && iparams && state && decided && pressed && table_scratch,
                 "dtmf_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "dtmf_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG((((uintptr_t)samples | (uintptr_t)state | (uintptr_t)table_scratch) & 3) == 0,
                 "dtmf_items: samples, state or table_scratch is not 4-byte aligned");
  DMEL_CHECK_ARG(row_stride >= 0 && out_pitch >= 0, "dtmf_items: negative row stride %lld or output pitch %lld", (long long)row_stride,
                 (long long)out_pitch);
  std::vector<uint32_t> tab((size_t)kDtmfWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x3fffffff, "dtmf_items: item %d: %lld new samples, expected 0 .. 2^30 - 1", s, (long long)n);
    if (n == 0) continue;                               // idle: its parameters are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(first[s] >= 0 && first[s] <= 0x3fffffff, "dtmf_items: item %d: first column %lld, expected 0 .. 2^30 - 1", s,
                   (long long)first[s]);
    const int32_t nb = N[s];
    DMEL_CHECK_ARG(nb >= kDtmfMinBlock && nb <= kDtmfMaxBlock, "dtmf_items: item %d: a block of %d samples, expected %d .. %d", s, nb,
                   kDtmfMinBlock, kDtmfMaxBlock);
    const int64_t most = (n + nb - 1) / nb;             // whatever the open block holds (at most N - 1 samples)
    DMEL_CHECK_ARG(out_pitch >= most, "dtmf_items: item %d: %lld samples can complete %lld blocks, which exceed the output pitch %lld", s,
                   (long long)n, (long long)most, (long long)out_pitch);
    const float* ck = coef + (size_t)8 * s;
    const float* fp = fparams + (size_t)5 * s;
    const int32_t* ip = iparams + (size_t)2 * s;
    for (int k = 0; k < 8; ++k)
      DMEL_CHECK_ARG(std::isfinite(ck[k]) && ck[k] >= -2.0f && ck[k] <= 2.0f, "dtmf_items: item %d: coefficient %d is not in [-2, 2]", s, k);
    for (int k = 0; k < 5; ++k)
      DMEL_CHECK_ARG(std::isfinite(fp[k]) && fp[k] > 0.0f, "dtmf_items: item %d: float parameter %d is not finite and positive", s, k);
    DMEL_CHECK_ARG(ip[0] >= 1 && ip[0] <= (1 << 20) && ip[1] >= 1 && ip[1] <= (1 << 20),
                   "dtmf_items: item %d: hits %d or misses %d outside [1, 2^20]", s, ip[0], ip[1]);
    uint32_t* it = tab.data() + (size_t)kDtmfWords * s;
    it[0] = (uint32_t)first[s]; it[1] = (uint32_t)n; it[2] = (uint32_t)nb;
    std::memcpy(it + 3, ck, 8 * sizeof(float));
    std::memcpy(it + 11, fp, 5 * sizeof(float));
    std::memcpy(it + 16, ip, 2 * sizeof(int32_t));
    ++live;
    bytes += 4.0 * (double)n + 2.0 * (double)most + 8.0 * kDtmfState;
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per detector launch (dmel_prof_read("dtmf"))
    ProfScope ps("small", st, 0.0, bytes), count("dtmf", st, 0.0, 0.0);
    hipLaunchKernelGGL(dtmf_kernel, dim3((unsigned)S), dim3(256), 0, st, samples, row_stride, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), decided, pressed, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- input level (block AGC) on codec-rate samples (include/dmel_hip.h: dmel_level_items; the rule and the state row: utils/level.py) --
// Row s of the table is (first, n_new, N, initial_gain, target, emin, min_gain, max_gain, attack, release, gate, ceiling, rN, 0, 0, 0),
// sixteen 4-byte words; workgroup s owns slot s and re-writes its new samples in place.  Positions are counted as in dtmf_kernel: the
// stream began `fill` samples in front of column `first`, block j of the launch holds positions [j N, (j + 1) N), of which
// [fill, fill + n_new) exist.  A pass takes min(64, 4096 / N) blocks (at least one) -- at most 4096 samples, the LDS tile -- through three
// phases with a barrier between them: (a) every live sample of the pass is read once into the tile, 16 bytes per lane on the aligned
// body of the range and single words on its head and tail (`first` is any column), and wave w reduces the raw peaks of blocks w,
// w + 4, ... from the tile (max is exact and order-free); (b) thread 0 runs the recursion of the pass's blocks in block order -- a few
// dozen scalar operations per block -- and leaves the two gains every block ramps between, and the outputs of the whole ones, in LDS;
// (c) every thread applies ramp, gain and clamp to its samples from the tile and stores them on the same 16-byte grid.  Nothing of a
// pass is stored before all of it is read, and passes do not overlap.  peak_out and clamped are reduced over the workgroup behind the
// last pass.  The ramp, the gain and the envelope step are separately rounded operations (fp contract(off), as dtmf_step above), the
// division is the correctly rounded one: what the fp32 host expression gives.  Plain stores, no atomics.
constexpr int kLevelWords = 16, kLevelState = 16, kLevelPassSamples = 4096, kLevelPassBlocks = 64;
constexpr int kLevelMinBlock = 32, kLevelMaxBlock = 4096;
__device__ __forceinline__ float level_apply(float x, float ga, float gb, int i, float rN, float ceiling, float& peak, int& clamped) {
#pragma clang fp contract(off)
  const float d = gb - ga;
  const float u = (float)(i + 1) * rN;
  const float m = d * u;
  const float gi = ga + m;
  float y = x * gi;
  if (y > ceiling) { y = ceiling; ++clamped; }
  else if (y < -ceiling) { y = -ceiling; ++clamped; }
  peak = fmaxf(peak, fabsf(y));
  return y;
}
__device__ __forceinline__ float level_envelope(float env, float p, float attack, float release) {
#pragma clang fp contract(off)
  const float k = p >= env ? attack : release;
  float t = p - env;
  t = k * t;
  return env + t;
}
__device__ __forceinline__ float level_gain(float env, float target, float emin, float gmin, float gmax) {
  const float e = env > emin ? env : emin;
  float g = target / e;
  g = g > gmin ? g : gmin;
  return g < gmax ? g : gmax;
}
__global__ __launch_bounds__(256) void level_kernel(float* __restrict__ samples, int64_t row_stride, const uint32_t* __restrict__ tab,
                                                    uint32_t* __restrict__ state, float* __restrict__ out_peak,
                                                    float* __restrict__ out_gain, int64_t out_pitch) {
  __shared__ float tile[kLevelPassSamples];
  __shared__ float bpk[kLevelPassBlocks], bga[kLevelPassBlocks], bgb[kLevelPassBlocks], bgo[kLevelPassBlocks];
  __shared__ float red_peak[4];
  __shared__ int red_clamped[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* row = tab + (size_t)s * kLevelWords;
  const int64_t n_new = (int64_t)(int32_t)row[1];
  if (n_new <= 0) return;                               // idle (uniform: in front of the first barrier)
  const int64_t first = (int64_t)(int32_t)row[0];
  const int N = (int)row[2];
  const float g0 = __uint_as_float(row[3]), target = __uint_as_float(row[4]), emin = __uint_as_float(row[5]);
  const float gmin = __uint_as_float(row[6]), gmax = __uint_as_float(row[7]), attack = __uint_as_float(row[8]);
  const float release = __uint_as_float(row[9]), gate = __uint_as_float(row[10]), ceiling = __uint_as_float(row[11]);
  const float rN = __uint_as_float(row[12]);
  uint32_t* srow = state + (size_t)s * kLevelState;
  int fill = (int)srow[6];
  if ((unsigned)fill >= (unsigned)N) fill = 0;          // no row the rule wrote; keeps every index below inside the launch's columns
  // the recursion's state: thread 0 alone advances it
  float env = __uint_as_float(srow[0]), open_peak = __uint_as_float(srow[3]), peak_in = __uint_as_float(srow[4]);
  int blocks = (int)srow[7], locked = (int)srow[8], held = (int)srow[9];
  float ga = locked ? __uint_as_float(srow[1]) : g0, gb = locked ? __uint_as_float(srow[2]) : g0;
  const int64_t end = fill + n_new;                     // positions [fill, end) exist
  const int64_t nblk = (end + N - 1) / N, done = end / N;
  float* src = samples + (int64_t)s * row_stride + first - fill;             // position p is src[p]; only [fill, end) is touched
  float* opk = out_peak + (int64_t)s * out_pitch;
  float* ogn = out_gain + (int64_t)s * out_pitch;
  const int PB = max(1, min(kLevelPassBlocks, kLevelPassSamples / N));
  float my_peak = 0.0f;
  int my_clamped = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += PB) {
    const int nb = (int)min((int64_t)PB, nblk - b0);
    const int nd = (int)max((int64_t)0, min((int64_t)nb, done - b0));          // the whole blocks of the pass
    const int64_t base = b0 * N;                        // tile[q] is position base + q; q in [lo, hi) exists
    const int lo = (int)(max((int64_t)fill, base) - base), hi = (int)(min(end, base + (int64_t)nb * N) - base);
    float* g = src + base;
    // the 16-byte grid of the range: `head` single words, nv vectors, the words from tail0 on
    const int head = min(hi - lo, (int)((4u - (unsigned)(((uintptr_t)(g + lo) >> 2) & 3u)) & 3u));
    const int nv = (hi - lo - head) >> 2, body = lo + head, tail0 = body + 4 * nv;
    // (a) every sample of the pass into the tile, then the raw peak of every block
    if (tid < head) tile[lo + tid] = g[lo + tid];
    for (int v = tid; v < nv; v += 256) {
      const int q = body + 4 * v;
      const float4 x = *reinterpret_cast<const float4*>(g + q);
      tile[q] = x.x; tile[q + 1] = x.y; tile[q + 2] = x.z; tile[q + 3] = x.w;
    }
    if (tid < hi - tail0) tile[tail0 + tid] = g[tail0 + tid];
    __syncthreads();
    for (int j = wave; j < nb; j += 4) {                // wave-uniform
      const int a = max(lo, j * N), z = min(hi, (j + 1) * N);
      float m = 0.0f;
      for (int q = a + lane; q < z; q += 64) m = fmaxf(m, fabsf(tile[q]));
      for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      if (lane == 0) bpk[j] = m;
    }
    __syncthreads();
    // (b) the recursion, in block order
    if (tid == 0) {
      for (int j = 0; j < nb; ++j) {
        bga[j] = ga; bgb[j] = gb;
        float p = bpk[j];
        if (b0 + j == 0) p = fmaxf(p, open_peak);       // the block that was open when the launch began
        if (j >= nd) { open_peak = p; break; }          // the block the launch leaves open (the last one)
        peak_in = fmaxf(peak_in, p);
        if (!locked) {
          if (p >= gate) { env = p; locked = 1; }
        } else if (p < gate && p < env) {
          held += 1;
        } else {
          env = level_envelope(env, p, attack, release);
        }
        const float gn = locked ? level_gain(env, target, emin, gmin, gmax) : g0;
        ga = gb; gb = gn; open_peak = 0.0f;
        blocks += 1;
        bpk[j] = p; bgo[j] = gn;
      }
    }
    __syncthreads();
    // (c) ramp, gain and clamp, from the tile to the row
    if (tid < head) {
      const int q = lo + tid, j = q / N;
      g[q] = level_apply(tile[q], bga[j], bgb[j], q - j * N, rN, ceiling, my_peak, my_clamped);
    }
    for (int v = tid; v < nv; v += 256) {
      const int q = body + 4 * v;
      int j = q / N, i = q - j * N;
      float y[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        y[k] = level_apply(tile[q + k], bga[j], bgb[j], i, rN, ceiling, my_peak, my_clamped);
        if (++i == N) { i = 0; ++j; }
      }
      *reinterpret_cast<float4*>(g + q) = make_float4(y[0], y[1], y[2], y[3]);
    }
    if (tid < hi - tail0) {
      const int q = tail0 + tid, j = q / N;
      g[q] = level_apply(tile[q], bga[j], bgb[j], q - j * N, rN, ceiling, my_peak, my_clamped);
    }
    if (tid < nd) {
      opk[b0 + tid] = bpk[tid];
      ogn[b0 + tid] = bgo[tid];
    }
    __syncthreads();                                    // the next pass overwrites the tile and the block tables
  }
  for (int o = 32; o; o >>= 1) {
    my_peak = fmaxf(my_peak, __shfl_xor(my_peak, o));
    my_clamped += __shfl_xor(my_clamped, o);
  }
  if (lane == 0) { red_peak[wave] = my_peak; red_clamped[wave] = my_clamped; }
  __syncthreads();
  if (tid == 0) {
    const float pk = fmaxf(fmaxf(red_peak[0], red_peak[1]), fmaxf(red_peak[2], red_peak[3]));
    const int cl = red_clamped[0] + red_clamped[1] + red_clamped[2] + red_clamped[3];
    srow[0] = __float_as_uint(env); srow[1] = __float_as_uint(ga); srow[2] = __float_as_uint(gb); srow[3] = __float_as_uint(open_peak);
    srow[4] = __float_as_uint(peak_in); srow[5] = __float_as_uint(fmaxf(__uint_as_float(srow[5]), pk));
    srow[6] = (uint32_t)(end - done * N); srow[7] = (uint32_t)blocks; srow[8] = (uint32_t)locked; srow[9] = (uint32_t)held;
    srow[10] = (uint32_t)((int)srow[10] + cl);
  }
}

}  // namespace dmel

extern "C" int dmel_level_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new, const int32_t* N,
                                const float* fparams, void* state, float* out_peak, float* out_gain, int64_t out_pitch,
                                void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(samples && first && n_new && N && fparams && state && out_peak && out_gain && table_scratch, "level_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "level_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG((((uintptr_t)samples | (uintptr_t)state | (uintptr_t)out_peak | (uintptr_t)out_gain | (uintptr_t)table_scratch) & 3) == 0,
                 "level_items: samples, state, out_peak, out_gain or table_scratch is not 4-byte aligned");
  DMEL_CHECK_ARG(row_stride >= 0 && out_pitch >= 0, "level_items: negative row stride %lld or output pitch %lld", (long long)row_stride,
                 (long long)out_pitch);
  static const char* const kNames[10] = {"initial_gain", "target", "emin", "min_gain", "max_gain", "attack", "release", "gate", "ceiling", "rN"};
  std::vector<uint32_t> tab((size_t)kLevelWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x3fffffff, "level_items: item %d: %lld new samples, expected 0 .. 2^30 - 1", s, (long long)n);
    if (n == 0) continue;                               // idle: its parameters are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(first[s] >= 0 && first[s] <= 0x3fffffff, "level_items: item %d: first column %lld, expected 0 .. 2^30 - 1", s,
                   (long long)first[s]);
    const int32_t nb = N[s];
    DMEL_CHECK_ARG(nb >= kLevelMinBlock && nb <= kLevelMaxBlock, "level_items: item %d: a block of %d samples, expected %d .. %d", s, nb,
                   kLevelMinBlock, kLevelMaxBlock);
    const int64_t most = (n + nb - 1) / nb;             // whatever the open block holds (at most N - 1 samples)
    DMEL_CHECK_ARG(out_pitch >= most, "level_items: item %d: %lld samples can complete %lld blocks, which exceed the output pitch %lld", s,
                   (long long)n, (long long)most, (long long)out_pitch);
    const float* fp = fparams + (size_t)10 * s;
    for (int k = 0; k < 10; ++k)                        // the gate alone may be 0
      DMEL_CHECK_ARG(std::isfinite(fp[k]) && (fp[k] > 0.0f || (k == 7 && fp[k] == 0.0f)),
                     "level_items: item %d: float parameter %d (%s) is not finite and positive", s, k, kNames[k]);
    DMEL_CHECK_ARG(fp[5] <= 1.0f && fp[6] <= 1.0f && fp[9] <= 1.0f, "level_items: item %d: attack %g, release %g or rN %g above 1", s,
                   (double)fp[5], (double)fp[6], (double)fp[9]);
    DMEL_CHECK_ARG(fp[3] <= fp[0] && fp[0] <= fp[4], "level_items: item %d: initial_gain %g outside [min_gain, max_gain] = [%g, %g]", s,
                   (double)fp[0], (double)fp[3], (double)fp[4]);
    uint32_t* it = tab.data() + (size_t)kLevelWords * s;
    it[0] = (uint32_t)first[s]; it[1] = (uint32_t)n; it[2] = (uint32_t)nb;
    std::memcpy(it + 3, fp, 10 * sizeof(float));
    ++live;
    bytes += 8.0 * (double)n + 8.0 * (double)most + 8.0 * kLevelState;
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per leveller launch (dmel_prof_read("level"))
    ProfScope ps("small", st, 0.0, bytes), count("level", st, 0.0, 0.0);
    hipLaunchKernelGGL(level_kernel, dim3((unsigned)S), dim3(256), 0, st, samples, row_stride, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), out_peak, out_gain, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- noise suppression (spectral gain) on codec-rate samples (include/dmel_hip.h: dmel_denoise_items; the rule, the constant table and
// the state row: utils/denoise.py).  Row s of the table is (first, n_new, N, learn_frames, alpha, oma, track, track_ratio, creep,
// floor_gain, eps, rN, 0, 0, 0, 0), sixteen 4-byte words; workgroup s owns slot s.  It takes the slot's state row, the window and the
// twiddles of its N (strided out of the constant table) into LDS once, then walks the new samples hop by hop: every thread reads x[p]
// into the raw window and stores the finished hop's sample to the same column; at a hop boundary the frame runs in LDS -- window,
// log2 N decimation-in-frequency stages (bin b ends at the bit-reversed index, so no permutation pass), the per-bin recursion on the
// bins 0 .. H with the mirrored bins written by the thread that owns the bin, log2 N decimation-in-time stages with the conjugate
// twiddles, window and overlap-add -- 2 log2 N + 5 barriers per frame.  The sums follow the rule's order (64 lane-strided partials, then
// the xor tree) and every wave computes them, so the silent-frame branch is uniform without a broadcast.  The samples are single
// words: a hop is at most two per thread, the frame's barriers are the cost, and the result cannot depend on where `first` lies.
// Every operation is rounded on its own (fp contract(off)), the divisions are the correctly rounded ones.  Plain stores, no atomics.
constexpr int kDnWords = 16, kDnMinN = 64, kDnMaxN = 1024, kDnMaxH = kDnMaxN / 2;
constexpr int kDnRaw = 16, kDnTail = kDnRaw + kDnMaxN, kDnHop = kDnTail + kDnMaxH, kDnNz = kDnHop + kDnMaxH, kDnPrev = kDnNz + kDnMaxH + 1;
constexpr int kDnState = (kDnPrev + kDnMaxH + 1 + 3) / 4 * 4;
constexpr int kDnTabCos = 2 * kDnMaxN, kDnTabSin = kDnTabCos + kDnMaxH;
__device__ __forceinline__ float denoise_sum(const float* v, int n, int lane) {
#pragma clang fp contract(off)
  float p = 0.0f;
  for (int b = lane; b < n; b += 64) p = p + v[b];
  for (int o = 32; o; o >>= 1) p = p + __shfl_xor(p, o);
  return p;
}
__global__ __launch_bounds__(256) void denoise_kernel(float* __restrict__ samples, int64_t row_stride, const uint32_t* __restrict__ tab,
                                                      uint32_t* __restrict__ state, float* __restrict__ out_in,
                                                      float* __restrict__ out_out, int64_t out_pitch,
                                                      const float* __restrict__ transform) {
#pragma clang fp contract(off)
  __shared__ float re[kDnMaxN], im[kDnMaxN], win[kDnMaxN], raw[kDnMaxN];
  __shared__ float twc[kDnMaxH], tws[kDnMaxH], tail[kDnMaxH], hop[kDnMaxH];
  __shared__ float nz[kDnMaxH + 1], prev[kDnMaxH + 1], pw[kDnMaxH + 1], qw[kDnMaxH + 1];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const uint32_t* row = tab + (size_t)s * kDnWords;
  const int64_t n_new = (int64_t)(int32_t)row[1];
  if (n_new <= 0) return;                               // idle (uniform: in front of the first barrier)
  const int64_t first = (int64_t)(int32_t)row[0];
  const int N = (int)row[2], H = N >> 1, r = kDnMaxN / N, bits = 31 - __clz(N), learn = (int)row[3];
  const float alpha = __uint_as_float(row[4]), oma = __uint_as_float(row[5]), track = __uint_as_float(row[6]);
  const float ratio = __uint_as_float(row[7]), creep = __uint_as_float(row[8]), floor_gain = __uint_as_float(row[9]);
  const float eps = __uint_as_float(row[10]), rN = __uint_as_float(row[11]);
  uint32_t* srow = state + (size_t)s * kDnState;
  float* frow = reinterpret_cast<float*>(srow);
  int frames = (int)srow[0], fill = (int)srow[1], learned = (int)srow[2];
  if ((unsigned)fill >= (unsigned)H) fill = 0;          // no row the rule wrote; keeps every index below inside the LDS arrays
  float sum_in = frow[3], sum_out = frow[4];
  for (int i = tid; i < N; i += 256) {
    raw[i] = frow[kDnRaw + i];
    win[i] = transform[(2 * i + 1) * r];
  }
  for (int i = tid; i < H; i += 256) {
    tail[i] = frow[kDnTail + i];
    hop[i] = frow[kDnHop + i];
    twc[i] = transform[kDnTabCos + i * r];
    tws[i] = transform[kDnTabSin + i * r];
  }
  for (int i = tid; i <= H; i += 256) {
    nz[i] = frow[kDnNz + i];
    prev[i] = frow[kDnPrev + i];
  }
  __syncthreads();
  float* g = samples + (int64_t)s * row_stride + first;  // the new samples are g[0 .. n_new)
  float* oin = out_in + (int64_t)s * out_pitch;
  float* oout = out_out + (int64_t)s * out_pitch;
  int64_t at = 0, done = 0;
  while (at < n_new) {
    const int m = (int)min((int64_t)(H - fill), n_new - at);
    for (int i = tid; i < m; i += 256) {                // in: the raw window; out: the hop the last frame finished, same column
      raw[H + fill + i] = g[at + i];
      g[at + i] = hop[fill + i];
    }
    at += m;
    fill += m;
    if (fill < H) break;                                // uniform
    __syncthreads();
    for (int i = tid; i < N; i += 256) {
      re[i] = raw[i] * win[i];
      im[i] = 0.0f;
    }
    for (int h = H; h >= 1; h >>= 1) {                  // forward: decimation in frequency
      __syncthreads();
      const int step = H / h;
      for (int t = tid; t < H; t += 256) {
        const int j = t & (h - 1), a = ((t - j) << 1) + j, b = a + h;
        const float wr = twc[j * step], wi = -tws[j * step];
        const float ar = re[a], ai = im[a], br = re[b], bi = im[b];
        const float dr = ar - br, di = ai - bi;
        re[a] = ar + br;
        im[a] = ai + bi;
        const float p0 = wr * dr, p1 = wi * di, p2 = wr * di, p3 = wi * dr;
        re[b] = p0 - p1;
        im[b] = p2 + p3;
      }
    }
    __syncthreads();
    for (int b = tid; b <= H; b += 256) {
      const int idx = (int)(__brev((unsigned)b) >> (32 - bits));
      const float xr = re[idx], xi = im[idx];
      const float p0 = xr * xr, p1 = xi * xi;
      float P = p0 + p1;
      if (P < 1e-30f) P = 0.0f;
      pw[b] = P;
    }
    __syncthreads();
    const float p_in = denoise_sum(pw, H + 1, lane);    // the same bits in every wave
    float p_out = 0.0f;
    const bool silent = p_in == 0.0f;                   // uniform
    if (!silent) {
      for (int b = tid; b <= H; b += 256) {
        const int idx = (int)(__brev((unsigned)b) >> (32 - bits));
        const float P = pw[b];
        float z = nz[b];
        if (learned < learn) {
          float d = P - z;
          d = d / (float)(learned + 1);
          z = z + d;
        } else {
          z = z * creep;
          const float t = ratio * z;
          if (P < t) {
            float d = P - z;
            d = track * d;
            z = z + d;
          }
        }
        nz[b] = z;
        const float den = z > eps ? z : eps;
        const float post = P / den;
        float e = post - 1.0f;
        e = e > 0.0f ? e : 0.0f;
        const float c0 = alpha * prev[b], c1 = oma * e;
        const float prio = c0 + c1;
        const float q = 1.0f + prio;
        float G = prio / q;
        G = G > floor_gain ? G : floor_gain;
        const float g2 = G * G;
        prev[b] = g2 * post;
        qw[b] = g2 * P;
        const float yr = G * re[idx], yi = G * im[idx];
        re[idx] = yr;
        im[idx] = yi;
        if (b > 0 && b < H) {
          const int mir = (int)(__brev((unsigned)(N - b)) >> (32 - bits));
          re[mir] = yr;
          im[mir] = -yi;
        }
      }
      if (learned < learn) ++learned;
      for (int h = 1; h <= H; h <<= 1) {                // inverse: decimation in time, conjugate twiddles
        __syncthreads();
        const int step = H / h;
        for (int t = tid; t < H; t += 256) {
          const int j = t & (h - 1), a = ((t - j) << 1) + j, b = a + h;
          const float wr = twc[j * step], wi = tws[j * step];
          const float ar = re[a], ai = im[a], br = re[b], bi = im[b];
          const float p0 = wr * br, p1 = wi * bi, p2 = wr * bi, p3 = wi * br;
          const float tr = p0 - p1, ti = p2 + p3;
          re[a] = ar + tr;
          im[a] = ai + ti;
          re[b] = ar - tr;
          im[b] = ai - ti;
        }
      }
      __syncthreads();
      p_out = denoise_sum(qw, H + 1, lane);
      sum_in = sum_in + p_in;
      sum_out = sum_out + p_out;
    }
    for (int i = tid; i < H; i += 256) {                // window, overlap-add, and the raw window moves on by one hop
      float v0 = 0.0f, v1 = 0.0f;
      if (!silent) {
        v0 = re[i] * rN;
        v0 = v0 * win[i];
        v1 = re[H + i] * rN;
        v1 = v1 * win[H + i];
      }
      const float o = tail[i] + v0;
      hop[i] = frames ? o : 0.0f;
      tail[i] = v1;
      raw[i] = raw[H + i];
    }
    if (tid == 0) {
      oin[done] = p_in;
      oout[done] = p_out;
    }
    ++frames;
    ++done;
    fill = 0;
    __syncthreads();                                    // the next hop streams out of `hop` and into `raw`
  }
  __syncthreads();
  const float nz_sum = denoise_sum(nz, H + 1, lane);
  for (int i = tid; i < N; i += 256) frow[kDnRaw + i] = raw[i];
  for (int i = tid; i < H; i += 256) {
    frow[kDnTail + i] = tail[i];
    frow[kDnHop + i] = hop[i];
  }
  for (int i = tid; i <= H; i += 256) {
    frow[kDnNz + i] = nz[i];
    frow[kDnPrev + i] = prev[i];
  }
  if (tid == 0) {
    srow[0] = (uint32_t)frames; srow[1] = (uint32_t)fill; srow[2] = (uint32_t)learned;
    frow[3] = sum_in; frow[4] = sum_out; frow[5] = nz_sum;
  }
}

}  // namespace dmel

extern "C" int dmel_denoise_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new, const int32_t* N,
                                  const int32_t* learn_frames, const float* fparams, void* state, float* power_in, float* power_out,
                                  int64_t out_pitch, const float* transform, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(samples && first && n_new && N && learn_frames && fparams && state && power_in && power_out && transform && table_scratch,
                 "denoise_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "denoise_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG((((uintptr_t)samples | (uintptr_t)state | (uintptr_t)power_in | (uintptr_t)power_out | (uintptr_t)transform |
                   (uintptr_t)table_scratch) & 3) == 0,
                 "denoise_items: samples, state, power_in, power_out, transform or table_scratch is not 4-byte aligned");
  DMEL_CHECK_ARG(row_stride >= 0 && out_pitch >= 0, "denoise_items: negative row stride %lld or output pitch %lld", (long long)row_stride,
                 (long long)out_pitch);
  static const char* const kNames[8] = {"alpha", "oma", "track", "track_ratio", "creep", "floor_gain", "eps", "rN"};
  static const float kLo[8] = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1e-6f, 1e-30f, 0.0f}, kHi[8] = {1.0f, 1.0f, 1.0f, 1e6f, 2.0f, 1.0f, 1.0f, 1.0f};
  std::vector<uint32_t> tab((size_t)kDnWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x3fffffff, "denoise_items: item %d: %lld new samples, expected 0 .. 2^30 - 1", s, (long long)n);
    if (n == 0) continue;                               // idle: its parameters are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(first[s] >= 0 && first[s] <= 0x3fffffff, "denoise_items: item %d: first column %lld, expected 0 .. 2^30 - 1", s,
                   (long long)first[s]);
    const int32_t nf = N[s];
    DMEL_CHECK_ARG(nf >= kDnMinN && nf <= kDnMaxN && (nf & (nf - 1)) == 0,
                   "denoise_items: item %d: a frame of %d samples, expected a power of two in %d .. %d", s, nf, kDnMinN, kDnMaxN);
    const int64_t hop = nf / 2, most = (n + hop - 1) / hop;                    // whatever the open hop holds (at most H - 1 samples)
    DMEL_CHECK_ARG(out_pitch >= most, "denoise_items: item %d: %lld samples can complete %lld frames, which exceed the output pitch %lld", s,
                   (long long)n, (long long)most, (long long)out_pitch);
    DMEL_CHECK_ARG(learn_frames[s] >= 1 && learn_frames[s] <= 4096, "denoise_items: item %d: learn_frames %d, expected 1 .. 4096", s,
                   learn_frames[s]);
    const float* fp = fparams + (size_t)8 * s;
    for (int k = 0; k < 8; ++k)
      DMEL_CHECK_ARG(std::isfinite(fp[k]) && fp[k] >= kLo[k] && fp[k] <= kHi[k],
                     "denoise_items: item %d: float parameter %d (%s) = %g is not finite or outside [%g, %g]", s, k, kNames[k], (double)fp[k],
                     (double)kLo[k], (double)kHi[k]);
    DMEL_CHECK_ARG(fp[0] < 1.0f && fp[1] > 0.0f && fp[2] > 0.0f, "denoise_items: item %d: alpha %g must be below 1, oma %g and track %g above 0",
                   s, (double)fp[0], (double)fp[1], (double)fp[2]);
    DMEL_CHECK_ARG(fp[7] * (float)nf == 1.0f, "denoise_items: item %d: rN %g is not 1 / %d", s, (double)fp[7], nf);
    uint32_t* it = tab.data() + (size_t)kDnWords * s;
    it[0] = (uint32_t)first[s]; it[1] = (uint32_t)n; it[2] = (uint32_t)nf; it[3] = (uint32_t)learn_frames[s];
    std::memcpy(it + 4, fp, 8 * sizeof(float));
    ++live;
    bytes += 8.0 * (double)n + 8.0 * (double)most + 8.0 * (double)(16 + 3 * nf + 2);
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per launch (dmel_prof_read("denoise"))
    ProfScope ps("small", st, 0.0, bytes), count("denoise", st, 0.0, 0.0);
    hipLaunchKernelGGL(denoise_kernel, dim3((unsigned)S), dim3(256), 0, st, samples, row_stride, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), power_in, power_out, out_pitch, transform);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- echo cancellation (block NLMS) on codec-rate samples (include/dmel_hip.h: dmel_echo_items; the rule and the state row: utils/echo.py)
// Row s of the table is (first, n_new, far pointer lo, hi, far_n, L, N, delay, mu, eps, far_floor, double_talk, meter, fN, 0, 0),
// sixteen 4-byte words; workgroup s owns slot s, appends the slot's new far samples to the ring in its state row and re-writes its new
// samples in place.  Positions are counted as in level_kernel: the stream began `fill` samples in front of column `first`, block j of
// the launch holds positions [j N, (j + 1) N), of which [fill, fill + n_new) exist.  A pass takes 2048 / N blocks through LDS: the far
// window of all of them (L - 1 samples of history in front), their d and e (the open block's first `fill` of each from the state row),
// then E and max |xd| of every block the pass completes -- 8 chains per block, all blocks at once, outside the serial part.  Then block
// by block, w fixed in LDS: (a) the (sample, segment) partial dots over the workgroup -- w[k] a broadcast read, xd[t - k] consecutive
// across lanes -- then the fixed tree, e to LDS and to the row; (b) wave 0 sums d^2 and e^2 (16 lanes, one chain each) and lane 0
// decides and computes the step; (c) every thread updates its taps k = tid + 256 r, eight chains over the block each.  w is read from
// the state row once and written once.  Every product and sum is rounded on its own (fp contract(off)); the division is the correctly
// rounded one.  Plain stores, no atomics.
constexpr int kEchoWords = 16, kEchoMinTaps = 64, kEchoMaxTaps = 2048, kEchoMinBlock = 16, kEchoMaxBlock = 256, kEchoMaxDelay = 24000;
constexpr int kEchoRing = 65536, kEchoPass = 2048;
constexpr int kEchoW = 16, kEchoE = kEchoW + kEchoMaxTaps, kEchoD = kEchoE + kEchoMaxBlock, kEchoFar = kEchoD + kEchoMaxBlock;
constexpr int kEchoRow = kEchoFar + kEchoRing;
constexpr int kEchoMaxAhead = kEchoRing - kEchoMaxDelay - kEchoMaxTaps - kEchoMaxBlock;
__device__ __forceinline__ float echo_tree(const float* s) {
  return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}
__global__ __launch_bounds__(256) void echo_kernel(float* __restrict__ samples, int64_t row_stride, const uint32_t* __restrict__ tab,
                                                   uint32_t* state, int64_t state_pitch, float* __restrict__ out_in,
                                                   float* __restrict__ out_res, int64_t out_pitch) {
#pragma clang fp contract(off)
  __shared__ float w[kEchoMaxTaps], xw[kEchoMaxTaps + kEchoPass], dl[kEchoPass], el[kEchoPass], part[2048];
  __shared__ float Eb[kEchoPass / kEchoMinBlock], mxb[kEchoPass / kEchoMinBlock];
  __shared__ float dec_step;
  __shared__ int dec_adapt, red_missing[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* row = tab + (size_t)s * kEchoWords;
  const int n_new = (int)row[1], far_n = (int)row[4];
  if (n_new <= 0 && far_n <= 0) return;                 // idle (uniform: in front of the first barrier)
  const int64_t first = (int64_t)(int32_t)row[0];
  const float* far = reinterpret_cast<const float*>(((uint64_t)row[3] << 32) | (uint64_t)row[2]);
  const int L = (int)row[5], N = (int)row[6], delay = (int)row[7];
  const float mu = __uint_as_float(row[8]), eps = __uint_as_float(row[9]), far_floor = __uint_as_float(row[10]);
  const float dtalk = __uint_as_float(row[11]), meter = __uint_as_float(row[12]), fN = __uint_as_float(row[13]);
  uint32_t* srow = state + (int64_t)s * state_pitch;
  float* frow = reinterpret_cast<float*>(srow);
  float* ring = frow + kEchoFar;
  const int64_t T = (int64_t)(int32_t)srow[0], F = (int64_t)(int32_t)srow[1];
  int fill = (int)srow[2];
  if ((unsigned)fill >= (unsigned)N) fill = 0;          // no row the rule wrote; keeps every index below inside the launch's columns
  // the far samples of the step: behind the ones the ring has; one whose turn has passed is dropped (its word holds the 0 of its turn)
  const int64_t room = T + kEchoMaxAhead - F;
  const int m = (int)max((int64_t)0, min((int64_t)far_n, room));
  for (int i = tid; i < m; i += 256) {
    const int64_t j = F + i;
    if (j >= T - delay) ring[j & (kEchoRing - 1)] = far[i];
  }
  const int64_t F2 = F + m;
  if (n_new <= 0) {                                     // far samples alone (uniform)
    if (tid == 0) srow[1] = (uint32_t)F2;
    return;
  }
  // a far sample that is not there at its turn reads as 0 from now on
  int my_missing = 0;
  for (int i = tid; i < n_new; i += 256) {
    const int64_t j = T + i - delay;
    if (j >= F2) { ring[j & (kEchoRing - 1)] = 0.0f; ++my_missing; }
  }
  for (int k = tid; k < L; k += 256) w[k] = frow[kEchoW + k];
  __syncthreads();
  // the recursion's state: thread 0 alone advances it
  float sd = __uint_as_float(srow[7]), se = __uint_as_float(srow[8]);
  int blocks = (int)srow[3], adapted = (int)srow[4], frozen = (int)srow[5];
  const int64_t end = (int64_t)fill + n_new;            // positions [fill, end) exist
  const int64_t nblk = (end + N - 1) / N, done = end / N;
  float* src = samples + (int64_t)s * row_stride + first - fill;              // position p is src[p]; only [fill, end) is touched
  float* oin = out_in + (int64_t)s * out_pitch;
  float* ores = out_res + (int64_t)s * out_pitch;
  const int PB = kEchoPass / N, n8 = N >> 3, l8 = L >> 3, nw = L + N - 1;
  for (int64_t b0 = 0; b0 < nblk; b0 += PB) {
    const int nb = (int)min((int64_t)PB, nblk - b0);
    const int nd = (int)max((int64_t)0, min((int64_t)nb, done - b0));          // the whole blocks of the pass
    const int64_t base = b0 * N;                        // dl[q] is position base + q; q in [lo, hi) is new
    const int lo = (int)(max((int64_t)fill, base) - base), hi = (int)(min(end, base + (int64_t)nb * N) - base);
    const int64_t j0 = T - fill + base - delay - (L - 1);                      // xw[q] = x[j0 + q]: xd of position q - (L - 1)
    for (int q = tid; q < L - 1 + hi; q += 256) {
      const int64_t j = j0 + q;
      xw[q] = j >= 0 ? ring[j & (kEchoRing - 1)] : 0.0f;
    }
    for (int q = tid; q < hi; q += 256) {
      if (q >= lo) {
        dl[q] = src[base + q];
      } else {                                          // the open block's samples of earlier launches (first pass only)
        dl[q] = frow[kEchoD + q];
        el[q] = frow[kEchoE + q];
      }
    }
    __syncthreads();
    // E and max |xd| of every whole block of the pass: chain (block c / 8, segment c % 8)
    for (int c = tid; c < nd * 8; c += 256) {
      const int q = c & 7;
      const float* v = xw + (c >> 3) * N;
      float acc = 0.0f, mx = 0.0f;
      for (int k = q * nw / 8, z = (q + 1) * nw / 8; k < z; ++k) {
        const float x = v[k];
        const float p = x * x;
        acc = acc + p;
        mx = fmaxf(mx, fabsf(x));
      }
      part[c] = acc;
      part[1024 + c] = mx;
    }
    __syncthreads();
    for (int j = tid; j < nd; j += 256) {
      Eb[j] = echo_tree(part + 8 * j);
      float mx = part[1024 + 8 * j];
      for (int q = 1; q < 8; ++q) mx = fmaxf(mx, part[1024 + 8 * j + q]);
      mxb[j] = mx;
    }
    __syncthreads();
    for (int jb = 0; jb < nb; ++jb) {
      const int pa = max(lo, jb * N), pz = min(hi, (jb + 1) * N), ni = pz - pa;   // the block's new positions
      // (a) partial dots: pair c is (sample c % ni, segment c / ni)
      for (int c = tid; c < ni * 8; c += 256) {
        const int seg = c / ni, i = c - seg * ni;
        const float* xv = xw + (L - 1) + pa + i;        // xv[-k] = xd[t - k]
        float acc = 0.0f;
        for (int k = seg * l8, z = k + l8; k < z; ++k) {
          const float p = w[k] * xv[-k];
          acc = acc + p;
        }
        part[seg * 256 + i] = acc;
      }
      __syncthreads();
      if (tid < ni) {
        float sg[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) sg[q] = part[q * 256 + tid];
        const float e = dl[pa + tid] - echo_tree(sg);
        el[pa + tid] = e;
        src[base + pa + tid] = e;
      }
      __syncthreads();
      if (jb >= nd) break;                              // the block the launch leaves open (the last one; uniform)
      // (b) the block's energies and the decision
      if (wave == 0) {
        const float* db = dl + jb * N;
        const float* eb = el + jb * N;
        float acc = 0.0f, md = 0.0f;
        if (lane < 16) {
          const float* v = lane < 8 ? db : eb;
          for (int i = (lane & 7) * n8, z = i + n8; i < z; ++i) {
            const float p = v[i] * v[i];
            acc = acc + p;
          }
        }
        for (int i = lane; i < N; i += 64) md = fmaxf(md, fabsf(db[i]));
        for (int o = 32; o; o >>= 1) md = fmaxf(md, __shfl_xor(md, o));
        float sa[8], sb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { sa[q] = __shfl(acc, q); sb[q] = __shfl(acc, 8 + q); }
        if (lane == 0) {
          const float Ed = echo_tree(sa), Ee = echo_tree(sb), E = Eb[jb];
          const float gt = dtalk * mxb[jb];
          const bool adapt = E >= far_floor && !(dtalk > 0.0f && md > gt);
          if (adapt) {
            float t = fN * E;
            t = t + eps;
            dec_step = mu / t;
            adapted += 1;
          } else {
            frozen += 1;
          }
          dec_adapt = adapt ? 1 : 0;
          float t = Ed - sd;
          t = meter * t;
          sd = sd + t;
          t = Ee - se;
          t = meter * t;
          se = se + t;
          blocks += 1;
          oin[b0 + jb] = Ed;
          ores[b0 + jb] = Ee;
        }
      }
      __syncthreads();
      // (c) the taps
      if (dec_adapt) {
        const float step = dec_step;
        const float* eb = el + jb * N;
        for (int k = tid; k < L; k += 256) {
          const float* xv = xw + (L - 1) + jb * N - k;  // xv[i] = xd[t0 + i - k]
          float sg[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
          for (int i = 0; i < n8; ++i) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const float p = eb[q * n8 + i] * xv[q * n8 + i];
              sg[q] = sg[q] + p;
            }
          }
          const float t = step * echo_tree(sg);
          w[k] = w[k] + t;
        }
      }
      __syncthreads();                                  // the next block reads w; the next decision overwrites dec_*
    }
    if (b0 + nb >= nblk) {                              // the last pass: the open block's d and e go to the state row, 0 behind them
      const int open = (int)(end - done * N), at = (int)(done * N - base);
      if (tid < kEchoMaxBlock) {
        frow[kEchoE + tid] = tid < open ? el[at + tid] : 0.0f;
        frow[kEchoD + tid] = tid < open ? dl[at + tid] : 0.0f;
      }
    }
    __syncthreads();                                    // the next pass overwrites the window and the block's rows
  }
  for (int k = tid; k < L; k += 256) frow[kEchoW + k] = w[k];
  for (int o = 32; o; o >>= 1) my_missing += __shfl_xor(my_missing, o);
  if (lane == 0) red_missing[wave] = my_missing;
  __syncthreads();
  if (tid == 0) {
    srow[0] = (uint32_t)(T + n_new); srow[1] = (uint32_t)F2; srow[2] = (uint32_t)(end - done * N); srow[3] = (uint32_t)blocks;
    srow[4] = (uint32_t)adapted; srow[5] = (uint32_t)frozen;
    srow[6] = (uint32_t)((int)srow[6] + red_missing[0] + red_missing[1] + red_missing[2] + red_missing[3]);
    srow[7] = __float_as_uint(sd); srow[8] = __float_as_uint(se);
  }
}

}  // namespace dmel

extern "C" int dmel_echo_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new,
                               const void* const* far, const int64_t* far_n, const int32_t* iparams, const float* fparams, void* state,
                               int64_t state_pitch, float* out_in, float* out_res, int64_t out_pitch, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(samples && first && n_new && far && far_n && iparams && fparams && state && out_in && out_res && table_scratch,
                 "echo_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "echo_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG((((uintptr_t)samples | (uintptr_t)state | (uintptr_t)out_in | (uintptr_t)out_res | (uintptr_t)table_scratch) & 3) == 0,
                 "echo_items: samples, state, out_in, out_res or table_scratch is not 4-byte aligned");
  DMEL_CHECK_ARG(row_stride >= 0 && out_pitch >= 0, "echo_items: negative row stride %lld or output pitch %lld", (long long)row_stride,
                 (long long)out_pitch);
  DMEL_CHECK_ARG(state_pitch >= kEchoRow, "echo_items: a state pitch of %lld words, expected at least %d", (long long)state_pitch, kEchoRow);
  static const char* const kNames[6] = {"mu", "eps", "far_floor", "double_talk", "meter", "fN"};
  std::vector<uint32_t> tab((size_t)kEchoWords * S, 0u);
  int64_t live = 0;
  double flops = 0.0, bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s], m = far_n[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x3fffffff, "echo_items: item %d: %lld new samples, expected 0 .. 2^30 - 1", s, (long long)n);
    DMEL_CHECK_ARG(m >= 0 && m <= 0x3fffffff, "echo_items: item %d: %lld far samples, expected 0 .. 2^30 - 1", s, (long long)m);
    if (n == 0 && m == 0) continue;                     // idle: its parameters are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(m == 0 || (far[s] && ((uintptr_t)far[s] & 3) == 0), "echo_items: item %d: %lld far samples at a NULL or unaligned pointer",
                   s, (long long)m);
    DMEL_CHECK_ARG(n == 0 || (first[s] >= 0 && first[s] <= 0x3fffffff), "echo_items: item %d: first column %lld, expected 0 .. 2^30 - 1", s,
                   (long long)first[s]);
    const int32_t L = iparams[3 * s], N = iparams[3 * s + 1], delay = iparams[3 * s + 2];
    DMEL_CHECK_ARG(L >= kEchoMinTaps && L <= kEchoMaxTaps && L % 64 == 0, "echo_items: item %d: %d taps, expected a multiple of 64 in %d .. %d",
                   s, L, kEchoMinTaps, kEchoMaxTaps);
    DMEL_CHECK_ARG(N >= kEchoMinBlock && N <= kEchoMaxBlock && N % 8 == 0,
                   "echo_items: item %d: a block of %d samples, expected a multiple of 8 in %d .. %d", s, N, kEchoMinBlock, kEchoMaxBlock);
    DMEL_CHECK_ARG(delay >= 0 && delay <= kEchoMaxDelay, "echo_items: item %d: a delay of %d samples, expected 0 .. %d", s, delay, kEchoMaxDelay);
    const int64_t most = (n + N - 1) / N;               // whatever the open block holds (at most N - 1 samples)
    DMEL_CHECK_ARG(out_pitch >= most, "echo_items: item %d: %lld samples can complete %lld blocks, which exceed the output pitch %lld", s,
                   (long long)n, (long long)most, (long long)out_pitch);
    const float* fp = fparams + (size_t)6 * s;
    for (int k = 0; k < 6; ++k)                         // far_floor and double_talk may be 0
      DMEL_CHECK_ARG(std::isfinite(fp[k]) && (fp[k] > 0.0f || ((k == 2 || k == 3) && fp[k] == 0.0f)),
                     "echo_items: item %d: float parameter %d (%s) is not finite and positive", s, k, kNames[k]);
    DMEL_CHECK_ARG(fp[0] < 2.0f && fp[4] <= 1.0f, "echo_items: item %d: mu %g is not below 2 or meter %g is above 1", s, (double)fp[0],
                   (double)fp[4]);
    DMEL_CHECK_ARG(fp[5] == (float)N, "echo_items: item %d: fN %g is not the block of %d samples", s, (double)fp[5], N);
    uint32_t* it = tab.data() + (size_t)kEchoWords * s;
    const uint64_t fptr = m ? (uint64_t)(uintptr_t)far[s] : 0;
    it[0] = (uint32_t)(n ? first[s] : 0); it[1] = (uint32_t)n; it[2] = (uint32_t)fptr; it[3] = (uint32_t)(fptr >> 32); it[4] = (uint32_t)m;
    it[5] = (uint32_t)L; it[6] = (uint32_t)N; it[7] = (uint32_t)delay;
    std::memcpy(it + 8, fp, 6 * sizeof(float));
    ++live;
    flops += 4.0 * (double)L * (double)n;               // the dots and the tap updates
    bytes += 8.0 * (double)n + 8.0 * (double)m + 8.0 * (double)most + 8.0 * (kEchoFar + L);
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per canceller launch (dmel_prof_read("echo"))
    ProfScope ps("small", st, flops, bytes), count("echo", st, 0.0, 0.0);
    hipLaunchKernelGGL(echo_kernel, dim3((unsigned)S), dim3(256), 0, st, samples, row_stride, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), state_pitch, out_in, out_res, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- packet-loss concealment (pitch repeat) on codec-rate samples (include/dmel_hip.h: dmel_conceal_items; the rule and the state
// row: utils/conceal.py).  Row s of the table is (first, n_new, n_ranges, W, Pmin, Pmax, H, D, F, floor, eps, rD, rF, 0, 0, 0) and
// behind them the 16 ranges (lo, hi), forty-eight 4-byte words; workgroup s owns slot s.  The ring of the slot's last 4096 output
// samples is read into LDS once and stays there for the launch; the header lives in registers, the same values in every thread.
// The row's stretches are walked in order, a barrier behind each, and each stretch is parallel:
//   good     the first `rec` samples are the recovery (below); the rest is a copy into the ring, the row is not written
//   onset    e0 by eight lanes; if the search runs, passes of 256 lags: the (lag, segment) partial sums of c and e over the workgroup
//            -- a[i] a broadcast read, b[i] consecutive across the lanes of one segment -- then one lag per thread: the fixed tree,
//            q, and the thread's running best; behind the passes a wave and a workgroup argmax on (q, -lag).  q is compared as a
//            value, so the order of the reduction cannot change the result
//   lost run, recovery   one lane per sample, 256 at a time: every source lies in front of t0.  A chunk reads, meets a barrier and
//            then writes: a write behind the fade may lap a ring word a sample in front of it still reads (H + D + Pmax == 4096),
//            and only samples of the same chunk can meet so, since reading samples precede writing ones
// At the end the ring words that changed and the header go back.  Every product, sum and division is rounded on its own
// (fp contract(off)); the division is the correctly rounded one.  Plain stores, no atomics.
constexpr int kConcealWords = 48, kConcealHeader = 16, kConcealRing = 4096, kConcealRow = kConcealHeader + kConcealRing;
constexpr int kConcealMaxRanges = 16, kConcealLagPass = 256;
__device__ __forceinline__ float conceal_synth(const float* ring, int t0, int P, int k, int H, int D, float rD) {
#pragma clang fp contract(off)
  if (P == 0 || k >= H + D) return 0.0f;
  const float v = ring[(unsigned)(t0 - P + k % P) & (kConcealRing - 1)];
  if (k < H) return v;
  const float u = (float)(k - H) * rD;
  const float g = 1.0f - u;
  return g * v;
}
__global__ __launch_bounds__(256) void conceal_kernel(float* __restrict__ samples, int64_t row_stride, const uint32_t* __restrict__ tab,
                                                      uint32_t* __restrict__ state, int64_t state_pitch, int32_t* __restrict__ out_period,
                                                      float* __restrict__ out_score, int64_t out_pitch) {
#pragma clang fp contract(off)
  __shared__ float ring[kConcealRing], pc[8 * kConcealLagPass], pe[8 * kConcealLagPass];
  __shared__ float red_q[4];
  __shared__ int red_p[4];
  constexpr unsigned M = kConcealRing - 1;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* row = tab + (size_t)s * kConcealWords;
  const int n_new = (int)row[1];
  if (n_new <= 0) return;                               // idle (uniform: in front of the first barrier)
  const int64_t first = (int64_t)(int32_t)row[0];
  const int nr = (int)row[2], W = (int)row[3], Pmin = (int)row[4], Pmax = (int)row[5], H = (int)row[6], D = (int)row[7], F = (int)row[8];
  const float floor_e = __uint_as_float(row[9]), eps = __uint_as_float(row[10]), rD = __uint_as_float(row[11]), rF = __uint_as_float(row[12]);
  const uint32_t* rg = row + 16;
  uint32_t* srow = state + (int64_t)s * state_pitch;
  float* frow = reinterpret_cast<float*>(srow);
  // the header: every thread advances its own copy, all alike
  int T = (int)srow[0], phase = (int)srow[1], t0 = (int)srow[2], P = (int)srow[3], k = (int)srow[4], rec = (int)srow[5];
  int lost = (int)srow[6], runs = (int)srow[7], muted = (int)srow[8], longest = (int)srow[9], run = (int)srow[10];
  float q = __uint_as_float(srow[11]), e0 = __uint_as_float(srow[12]);
  if (P < 0 || P > Pmax) P = 0;                         // no row the rule wrote; keeps k % P and the reads inside the ring
  if (rec < 0 || rec > F) rec = 0;
  for (int i = tid; i < kConcealRing; i += 256) ring[i] = frow[kConcealHeader + i];
  __syncthreads();
  float* src = samples + (int64_t)s * row_stride + first;                     // only [0, n_new) is touched
  int32_t* oper = out_period + (int64_t)s * out_pitch;
  float* osc = out_score + (int64_t)s * out_pitch;
  const int T_in = T, w8 = W >> 3;
  int pos = 0, onsets = 0;
  for (int ri = 0; ri <= nr; ++ri) {
    const int lo = ri < nr ? (int)rg[2 * ri] : n_new, hi = ri < nr ? (int)rg[2 * ri + 1] : n_new;
    if (pos < lo) {                                     // a good stretch [pos, lo)
      if (phase == 1) { longest = max(longest, run); phase = 2; rec = F; }
      const int len = lo - pos, r = phase == 2 ? min(rec, len) : 0;
      for (int j0 = 0; j0 < r; j0 += 256) {             // the recovery: the cross-fade from s(k) into x
        const int j = j0 + tid;
        float y = 0.0f;
        if (j < r) {
          const float x = src[pos + j];
          const float sv = conceal_synth(ring, t0, P, k + j, H, D, rD);
          const float w = (float)(F - rec + j + 1) * rF;
          const float d = x - sv;
          const float m = w * d;
          y = sv + m;
        }
        __syncthreads();
        if (j < r) {
          ring[(unsigned)(T + j) & M] = y;
          src[pos + j] = y;
        }
      }
      for (int j = r + tid; j < len; j += 256) ring[(unsigned)(T + j) & M] = src[pos + j];
      if (r) {
        k += r; rec -= r;
        if (rec == 0) phase = 0;
      }
      T += len; pos = lo;
      __syncthreads();
    }
    if (lo == hi) break;                                // behind the last range
    if (phase != 1) {                                   // the onset
      t0 = T; k = 0; P = 0; run = 0; runs += 1; phase = 1; q = 0.0f; e0 = 0.0f;
      if (T >= W + Pmax) {
        if (tid < 8) {
          float acc = 0.0f;
          for (int i = tid * w8, z = i + w8; i < z; ++i) {
            const float a = ring[(unsigned)(t0 - W + i) & M];
            const float p = a * a;
            acc = acc + p;
          }
          pc[tid] = acc;
        }
        __syncthreads();
        e0 = echo_tree(pc);
        __syncthreads();                                // the passes overwrite pc
        if (e0 >= floor_e) {
          float bq = 0.0f;
          int bp = 0;
          const int nl = Pmax - Pmin + 1;
          for (int l0 = 0; l0 < nl; l0 += kConcealLagPass) {
            const int cnt = min(kConcealLagPass, nl - l0);
            for (int c = tid; c < cnt * 8; c += 256) {  // pair c is (segment c / cnt, lag Pmin + l0 + c % cnt)
              const int seg = c / cnt, li = c - seg * cnt, p = Pmin + l0 + li;
              const int at = t0 - W + seg * w8;
              float ac = 0.0f, ae = 0.0f;
              for (int i = 0; i < w8; ++i) {
                const float a = ring[(unsigned)(at + i) & M], b = ring[(unsigned)(at + i - p) & M];
                const float ab = a * b;
                ac = ac + ab;
                const float bb = b * b;
                ae = ae + bb;
              }
              pc[seg * kConcealLagPass + li] = ac;
              pe[seg * kConcealLagPass + li] = ae;
            }
            __syncthreads();
            if (tid < cnt) {
              float sc[8], se[8];
#pragma unroll
              for (int g = 0; g < 8; ++g) { sc[g] = pc[g * kConcealLagPass + tid]; se[g] = pe[g * kConcealLagPass + tid]; }
              const float c = echo_tree(sc), e = echo_tree(se);
              float qv = 0.0f;
              if (c > 0.0f) {
                const float cc = c * c;
                const float ee = e + eps;
                qv = cc / ee;
              }
              if (qv > bq) { bq = qv; bp = Pmin + l0 + tid; }     // a thread's lags ascend: the lowest of equal ones stays
            }
            __syncthreads();
          }
          for (int o = 32; o; o >>= 1) {
            const float oq = __shfl_xor(bq, o);
            const int op = __shfl_xor(bp, o);
            if (oq > bq || (oq == bq && op < bp)) { bq = oq; bp = op; }
          }
          if (lane == 0) { red_q[wave] = bq; red_p[wave] = bp; }
          __syncthreads();
          bq = red_q[0]; bp = red_p[0];
          for (int v = 1; v < 4; ++v)
            if (red_q[v] > bq || (red_q[v] == bq && red_p[v] < bp)) { bq = red_q[v]; bp = red_p[v]; }
          q = bq;
          P = bq > 0.0f ? bp : 0;
        }
      }
      if (tid == 0) { oper[onsets] = P; osc[onsets] = q; }
      ++onsets;
    }
    const int m = hi - lo;                              // the lost stretch [lo, hi)
    for (int j0 = 0; j0 < m; j0 += 256) {
      const int j = j0 + tid;
      const float y = j < m ? conceal_synth(ring, t0, P, k + j, H, D, rD) : 0.0f;
      __syncthreads();
      if (j < m) {
        ring[(unsigned)(T + j) & M] = y;
        src[pos + j] = y;
      }
    }
    muted += P == 0 ? m : max(0, k + m - max(k, H + D));
    k += m; lost += m; run += m; T += m; pos = hi;
    __syncthreads();
  }
  // the ring words the launch wrote, then the header
  const int changed = min(n_new, kConcealRing);
  for (int i = tid; i < changed; i += 256) {
    const unsigned at = (unsigned)(T - changed + i) & M;
    frow[kConcealHeader + at] = ring[at];
  }
  if (tid == 0) {
    srow[0] = (uint32_t)(T_in + n_new); srow[1] = (uint32_t)phase; srow[2] = (uint32_t)t0; srow[3] = (uint32_t)P; srow[4] = (uint32_t)k;
    srow[5] = (uint32_t)rec; srow[6] = (uint32_t)lost; srow[7] = (uint32_t)runs; srow[8] = (uint32_t)muted; srow[9] = (uint32_t)longest;
    srow[10] = (uint32_t)run; srow[11] = __float_as_uint(q); srow[12] = __float_as_uint(e0);
  }
}

}  // namespace dmel

extern "C" int dmel_conceal_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new,
                                  const int32_t* n_ranges, const int32_t* ranges, const int32_t* iparams, const float* fparams, void* state,
                                  int64_t state_pitch, int32_t* out_period, float* out_score, int64_t out_pitch, void* table_scratch,
                                  void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(samples && first && n_new && n_ranges && ranges && iparams && fparams && state && out_period && out_score && table_scratch,
                 "conceal_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "conceal_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG((((uintptr_t)samples | (uintptr_t)state | (uintptr_t)out_period | (uintptr_t)out_score | (uintptr_t)table_scratch) & 3) == 0,
                 "conceal_items: samples, state, out_period, out_score or table_scratch is not 4-byte aligned");
  DMEL_CHECK_ARG(row_stride >= 0 && out_pitch >= 0, "conceal_items: negative row stride %lld or output pitch %lld", (long long)row_stride,
                 (long long)out_pitch);
  DMEL_CHECK_ARG(state_pitch >= kConcealRow, "conceal_items: a state pitch of %lld words, expected at least %d", (long long)state_pitch,
                 kConcealRow);
  std::vector<uint32_t> tab((size_t)kConcealWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x3fffffff, "conceal_items: item %d: %lld new samples, expected 0 .. 2^30 - 1", s, (long long)n);
    if (n == 0) continue;                               // idle: its parameters are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(first[s] >= 0 && first[s] <= 0x3fffffff, "conceal_items: item %d: first column %lld, expected 0 .. 2^30 - 1", s,
                   (long long)first[s]);
    const int32_t nr = n_ranges[s];
    DMEL_CHECK_ARG(nr >= 0 && nr <= kConcealMaxRanges, "conceal_items: item %d: %d lost ranges, expected 0 .. %d", s, nr, kConcealMaxRanges);
    DMEL_CHECK_ARG(out_pitch >= nr, "conceal_items: item %d: %d lost ranges can be %d onsets, which exceed the output pitch %lld", s, nr, nr,
                   (long long)out_pitch);
    const int32_t* rg = ranges + (size_t)2 * kConcealMaxRanges * s;
    int64_t lost = 0;
    for (int r = 0; r < nr; ++r) {
      const int32_t lo = rg[2 * r], hi = rg[2 * r + 1];
      DMEL_CHECK_ARG(lo >= 0 && lo < hi && hi <= n, "conceal_items: item %d: range %d is [%d, %d), expected a part of [0, %lld]", s, r, lo, hi,
                     (long long)n);
      DMEL_CHECK_ARG(r == 0 || lo > rg[2 * r - 1], "conceal_items: item %d: range %d begins at %d, not behind the end %d of the one before: "
                     "ranges are sorted and do not touch", s, r, lo, r ? rg[2 * r - 1] : 0);
      lost += hi - lo;
    }
    const int32_t* ip = iparams + (size_t)6 * s;
    const int32_t W = ip[0], Pmin = ip[1], Pmax = ip[2], H = ip[3], D = ip[4], F = ip[5];
    DMEL_CHECK_ARG(W >= 8 && W % 8 == 0, "conceal_items: item %d: a window of %d samples, expected a multiple of 8, at least 8", s, W);
    DMEL_CHECK_ARG(Pmin >= 8 && Pmin <= Pmax, "conceal_items: item %d: a lag range of [%d, %d], expected 8 <= Pmin <= Pmax", s, Pmin, Pmax);
    DMEL_CHECK_ARG((int64_t)W + Pmax <= kConcealRing, "conceal_items: item %d: a window of %d and a longest period of %d exceed the ring of %d",
                   s, W, Pmax, kConcealRing);
    DMEL_CHECK_ARG(H >= 0 && D >= 0 && (int64_t)H + D + Pmax <= kConcealRing,
                   "conceal_items: item %d: a hold of %d, a fade of %d and a longest period of %d exceed the ring of %d", s, H, D, Pmax,
                   kConcealRing);
    DMEL_CHECK_ARG(F >= 1 && F <= 0x3fffffff, "conceal_items: item %d: a recovery of %d samples, expected at least 1", s, F);
    const float* fp = fparams + (size_t)4 * s;
    DMEL_CHECK_ARG(std::isfinite(fp[0]) && fp[0] >= 0.0f && std::isfinite(fp[2]) && fp[2] >= 0.0f,
                   "conceal_items: item %d: floor %g or rD %g is not finite or is negative", s, (double)fp[0], (double)fp[2]);
    DMEL_CHECK_ARG(std::isfinite(fp[1]) && fp[1] > 0.0f && std::isfinite(fp[3]) && fp[3] > 0.0f && fp[3] <= 1.0f,
                   "conceal_items: item %d: eps %g or rF %g is not finite and positive, or rF is above 1", s, (double)fp[1], (double)fp[3]);
    uint32_t* it = tab.data() + (size_t)kConcealWords * s;
    it[0] = (uint32_t)first[s]; it[1] = (uint32_t)n; it[2] = (uint32_t)nr;
    std::memcpy(it + 3, ip, 6 * sizeof(int32_t));
    std::memcpy(it + 9, fp, 4 * sizeof(float));
    std::memcpy(it + 16, rg, (size_t)2 * nr * sizeof(int32_t));
    ++live;
    bytes += 4.0 * (double)n + 4.0 * (double)lost + 8.0 * (double)nr + 4.0 * (kConcealRow + std::min<double>((double)n, kConcealRing));
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per concealment launch (dmel_prof_read("conceal"))
    ProfScope ps("small", st, 0.0, bytes), count("conceal", st, 0.0, 0.0);
    hipLaunchKernelGGL(conceal_kernel, dim3((unsigned)S), dim3(256), 0, st, samples, row_stride, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), state_pitch, out_period, out_score, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- tones spliced into codec-rate audio (include/dmel_hip.h: dmel_tone_items; the rule: utils/tones.py) -----------------------------
// The table holds R part rows of (dst, src, n, first tile, first segment record, segments), six int64, and behind them the launch's
// segment records of five int64: the eight 4-byte words of the entry's table (f1, f2, a1, a2, on, off, ramp, ramp_off) and the
// segment's first sample inside its part -- the part's prefix sums (one record per segment: the entry refuses a segment that two
// parts would begin at different samples).  A workgroup owns one tile of kToneTile floats of the part that
// owns tile blockIdx.x: the last one whose first tile is not behind it, as in stream_pack_kernel (an idle part owns no tile).  Tiles
// are laid on the 16-byte grid of the DESTINATION: a lane owns the four floats of one aligned 16 bytes, so that every lane but the
// two that meet the ends of a part stores one float4, whatever the offset of dst; those two store their floats one by one.  A copy
// part loads a float4 where the source shares the destination's offset and single words else; words move as uint32.  A tone part
// finds the segment of its first sample by bisection over the records' first samples and steps on from there.  The four operations
// of a sample are rounded one by one (fp contract(off) in tone_sample, as in fade_blend above).  No LDS, no atomics.
constexpr int kTonePartWords = 6, kToneSegWords = 5, kToneTile = 1024, kToneMaxSegs = 64, kToneMaxRamp = 4096;
__device__ __forceinline__ float tone_sample(float a1, float s1, float a2, float s2, float g) {
#pragma clang fp contract(off)
  const float t1 = a1 * s1;
  const float t2 = a2 * s2;
  const float x = t1 + t2;
  return x * g;
}
__global__ __launch_bounds__(256) void tone_kernel(const int64_t* __restrict__ tab, int R, const float* __restrict__ sine, int rate,
                                                   const float* __restrict__ ramps) {
  const int64_t tile = blockIdx.x;
  int a = 0, b = R - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (tab[(size_t)mid * kTonePartWords + 3] <= tile) a = mid;
    else b = mid - 1;
  }
  const int64_t* row = tab + (size_t)a * kTonePartWords;
  uint32_t* dst = reinterpret_cast<uint32_t*>(row[0]);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(row[1]);
  const int64_t n = row[2], local = tile - row[3];
  if (n <= 0 || local < 0) return;
  const int shift = (int)((row[0] >> 2) & 3);                                // floats of dst past a 16-byte boundary
  const int64_t e = local * kToneTile + 4 * (int64_t)threadIdx.x - shift;    // dst + e is 16-byte aligned
  if (e >= n || e + 4 <= 0) return;
  const bool whole = e >= 0 && e + 4 <= n;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  if (src) {
    if (whole && (reinterpret_cast<uintptr_t>(src + e) & 15) == 0) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + e);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j >= 0 && e + j < n) v[j] = src[e + j];
    }
  } else {
    const int64_t* segs = tab + (size_t)R * kTonePartWords + (size_t)row[4] * kToneSegWords;
    const int count = (int)row[5];
    const int64_t lo = e < 0 ? 0 : e;
    int k = 0, kb = count - 1;
    while (k < kb) {
      const int mid = (k + kb + 1) >> 1;
      if (segs[(size_t)mid * kToneSegWords + 4] <= lo) k = mid;
      else kb = mid - 1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t t = e + j;
      if (t < 0 || t >= n) continue;
      while (k + 1 < count && segs[(size_t)(k + 1) * kToneSegWords + 4] <= t) ++k;
      const int32_t* w = reinterpret_cast<const int32_t*>(segs + (size_t)k * kToneSegWords);
      const int64_t i = t - segs[(size_t)k * kToneSegWords + 4];
      const int on = w[4], ramp = w[6];
      float y = 0.0f;                                                       // the gap behind the sound
      if (i < on) {
        const uint32_t p1 = (uint32_t)(((uint64_t)(uint32_t)w[0] * (uint64_t)i) % (uint64_t)rate);
        const uint32_t p2 = (uint32_t)(((uint64_t)(uint32_t)w[1] * (uint64_t)i) % (uint64_t)rate);
        float g = 1.0f;
        if (i < ramp) g = ramps[(int64_t)w[7] + i];
        else if (i >= on - ramp) g = ramps[(int64_t)w[7] + (on - 1 - i)];
        y = tone_sample(__int_as_float(w[2]), sine[p1], __int_as_float(w[3]), sine[p2], g);
      }
      v[j] = __float_as_uint(y);
    }
  }
  if (whole) {
    *reinterpret_cast<uint4*>(dst + e) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e + j >= 0 && e + j < n) dst[e + j] = v[j];
  }
}

}  // namespace dmel

extern "C" int dmel_tone_items(float* const* dst, const float* const* src, const int64_t* n, const int32_t* seg_first,
                               const int32_t* seg_count, int R, const int32_t* segs, int n_segs, const float* sine, int rate,
                               const float* ramps, int64_t ramp_floats, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(dst && src && n && seg_first && seg_count && sine && table_scratch, "tone_items: NULL argument");
  DMEL_CHECK_ARG(R >= 1 && R <= 65535, "tone_items: %d parts, expected 1 .. 65535", R);
  DMEL_CHECK_ARG(n_segs >= 0 && n_segs <= kToneMaxSegs * 65535 && (segs || n_segs == 0),
                 "tone_items: a segment table of %d segments (NULL: %d), expected 0 .. %d", n_segs, (int)!segs, kToneMaxSegs * 65535);
  DMEL_CHECK_ARG(rate >= 4000 && rate <= 192000, "tone_items: a rate of %d Hz, expected 4000 .. 192000", rate);
  DMEL_CHECK_ARG(ramp_floats >= 0 && (ramps || ramp_floats == 0), "tone_items: a ramp arena of %lld floats (NULL: %d)",
                 (long long)ramp_floats, (int)!ramps);
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 7) == 0, "tone_items: table_scratch is not 8-byte aligned");
  DMEL_CHECK_ARG((((uintptr_t)sine | (uintptr_t)ramps) & 3) == 0, "tone_items: sine or ramps is not 4-byte aligned");
  std::vector<int64_t> tab((size_t)kTonePartWords * R + (size_t)kToneSegWords * n_segs);
  int64_t* rec = tab.data() + (size_t)kTonePartWords * R;
  std::vector<int64_t> claimed((size_t)n_segs, -1);   // the first sample a part has given the segment's record (-1: none has)
  const int64_t limit = (int64_t)1 << 40;
  int64_t tiles = 0;
  double bytes = 0.0;
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(n[r] >= 0 && n[r] < limit, "tone_items: part %d: %lld samples, expected 0 .. 2^40 - 1", r, (long long)n[r]);
    int64_t* it = tab.data() + (size_t)kTonePartWords * r;
    it[3] = tiles;
    if (n[r] == 0) continue;                            // idle: its pointers and segments are not looked at (the table row stays 0)
    DMEL_CHECK_ARG(dst[r], "tone_items: part %d: NULL destination", r);
    DMEL_CHECK_ARG((((uintptr_t)dst[r] | (uintptr_t)src[r]) & 3) == 0, "tone_items: part %d: a pointer is not 4-byte aligned", r);
    it[0] = (int64_t)(uintptr_t)dst[r]; it[1] = (int64_t)(uintptr_t)src[r]; it[2] = n[r];
    if (!src[r]) {
      const int first = seg_first[r], count = seg_count[r];
      DMEL_CHECK_ARG(count >= 1 && count <= kToneMaxSegs && first >= 0 && first <= n_segs - count,
                     "tone_items: part %d: segments [%d, %d + %d) of a table of %d, expected 1 .. %d segments inside it", r, first, first,
                     count, n_segs, kToneMaxSegs);
      int64_t at = 0;
      for (int k = first; k < first + count; ++k) {
        const int32_t* w = segs + (size_t)8 * k;
        float amp[2];
        std::memcpy(amp, w + 2, sizeof(amp));
        for (int j = 0; j < 2; ++j) {
          DMEL_CHECK_ARG(w[j] >= 0 && 2 * (int64_t)w[j] < rate, "tone_items: part %d: segment %d: f%d = %d Hz, expected 0 <= f < %d / 2", r,
                         k, j + 1, w[j], rate);
          DMEL_CHECK_ARG(std::isfinite(amp[j]) && amp[j] >= 0.0f && (w[j] != 0 || amp[j] == 0.0f),
                         "tone_items: part %d: segment %d: amplitude a%d = %g is not finite and >= 0, or not 0 with f%d = 0", r, k, j + 1,
                         (double)amp[j], j + 1);
        }
        DMEL_CHECK_ARG((double)amp[0] + (double)amp[1] <= 1.0, "tone_items: part %d: segment %d: amplitudes %g + %g exceed 1", r, k,
                       (double)amp[0], (double)amp[1]);
        const int on = w[4], off = w[5], ramp = w[6], ramp_off = w[7];
        DMEL_CHECK_ARG(on >= 1 && on < (1 << 24) && off >= 0 && off < (1 << 24),
                       "tone_items: part %d: segment %d: on = %d, off = %d, expected 1 <= on < 2^24 and 0 <= off < 2^24", r, k, on, off);
        DMEL_CHECK_ARG(ramp >= 0 && ramp <= on / 2 && ramp <= kToneMaxRamp,
                       "tone_items: part %d: segment %d: ramp = %d, expected 0 .. min(on / 2, %d)", r, k, ramp, kToneMaxRamp);
        DMEL_CHECK_ARG(ramp == 0 || (ramp_off >= 0 && (int64_t)ramp_off + ramp <= ramp_floats),
                       "tone_items: part %d: segment %d: ramp table [%d, %d + %d) lies beyond the arena of %lld floats", r, k, ramp_off,
                       ramp_off, ramp, (long long)ramp_floats);
        // one record per segment of the table: parts may share segments only where each segment begins at the same sample in both
        DMEL_CHECK_ARG(claimed[k] < 0 || claimed[k] == at,
                       "tone_items: part %d: segment %d begins at sample %lld of this part and at sample %lld of an earlier one: parts "
                       "may share a segment only at one offset", r, k, (long long)at, (long long)claimed[k]);
        claimed[k] = at;
        int64_t* q = rec + (size_t)kToneSegWords * k;
        std::memcpy(q, w, 8 * sizeof(int32_t));
        q[4] = at;
        at += (int64_t)on + off;
      }
      DMEL_CHECK_ARG(at == n[r], "tone_items: part %d: its %d segments are %lld samples long, the part %lld: a length mismatch", r, count,
                     (long long)at, (long long)n[r]);
      it[4] = first; it[5] = count;
      bytes += 4.0 * (double)n[r];
    } else {
      bytes += 8.0 * (double)n[r];
    }
    const int64_t shift = (int64_t)(((uintptr_t)dst[r] >> 2) & 3);
    tiles += (n[r] + shift + kToneTile - 1) / kToneTile;
    DMEL_CHECK_ARG(tiles <= 0x7fffffff, "tone_items: part %d: more than 2^31 - 1 tiles", r);
  }
  if (tiles == 0) return DMEL_OK;                       // every part idle
  hipStream_t s = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(int64_t), table_scratch, s));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per tone launch (dmel_prof_read("tones"))
    ProfScope ps("small", s, 0.0, bytes), count("tones", s, 0.0, 0.0);
    hipLaunchKernelGGL(tone_kernel, dim3((unsigned)tiles), dim3(256), 0, s, static_cast<const int64_t*>(table_scratch), R, sine, rate, ramps);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- reply shaping on codec-rate audio (include/dmel_hip.h: dmel_shape_items; the rule and the state row: utils/shape.py) --------------
// Row s of the table is 64 4-byte words: dst (2), src (2), n_new, hold, flags (1: final, 2: limit), N, ceiling, release, rN, base,
// segment count, three zeros, then eight segment records of five words (start relative to the first new sample, ramp, ramp_off, g0,
// g1); workgroup s owns slot s.  The slot's LOCAL stream is its `hold` held samples of v (from its state row) followed by the n_new new
// ones, v = z * c; local block j holds local positions [j N, (j + 1) N).  A pass takes PB + 1 consecutive blocks (PB = min(63,
// 4096 / N), at most 5120 floats) through LDS and emits the first PB of them; the next pass begins at the block the last one kept, so
// every block's successor is in the tile when it leaves.  Phases of a pass, a barrier between them: (a) the held samples from the row
// and the new ones from src -- 16 bytes per lane on the aligned body, single words at the ends (src is any 4-byte offset), the
// commanded gain by a walk over the slot's segments -- into the tile; (b) wave w reduces the peaks of blocks w, w + 4, ...; (c) thread 0
// runs the s / n recursion over the blocks the pass completes, in block order, and leaves every block's start node in LDS; (d) ramp,
// gain and clamp from the tile to dst on the 16-byte grid of dst (another buffer than src: the counts differ); (e) behind the last
// pass the samples that did not leave go back to the row, and the rest of its hold is zeroed.  Without the limiter the same passes run
// with every node 1.0f (v * 1.0f is v) and nothing held.  Every operation of the rule is rounded on its own (fp contract(off)).  Plain
// stores, no atomics.
constexpr int kShapeWords = 64, kShapeHeader = 16, kShapeMinBlock = 32, kShapeMaxBlock = 1024, kShapePassSamples = 4096;
constexpr int kShapePassBlocks = 63, kShapeTile = kShapePassSamples + kShapeMaxBlock, kShapeMaxSegs = 8, kShapeSegWords = 5;
constexpr int kShapeMaxRamp = 16384, kShapeSegBase = 16, kShapeFparams = 5;
__device__ __forceinline__ float shape_gain(const uint32_t* seg, int nseg, float base, const float* __restrict__ ramps, int i) {
#pragma clang fp contract(off)
  int k = -1;
  for (int q = 0; q < nseg; ++q)
    if ((int)seg[q * kShapeSegWords] <= i) k = q;         // starts do not decrease: the last one at or in front of i
  if (k < 0) return base;
  const uint32_t* w = seg + k * kShapeSegWords;
  const int at = i - (int)w[0], ramp = (int)w[1];
  const float g1 = __uint_as_float(w[4]);
  if (at >= ramp) return g1;
  const float g0 = __uint_as_float(w[3]);
  const float d = g1 - g0;
  const float m = d * ramps[(int)w[2] + at];
  return g0 + m;
}
__device__ __forceinline__ float shape_apply(float v, float na, float nb, int i, float rN, float ceiling, float& peak, int& clamped) {
#pragma clang fp contract(off)
  const float d = nb - na;
  const float u = (float)(i + 1) * rN;
  const float m = d * u;
  const float gi = na + m;
  float y = v * gi;
  if (y > ceiling) { y = ceiling; ++clamped; }
  else if (y < -ceiling) { y = -ceiling; ++clamped; }
  peak = fmaxf(peak, fabsf(y));
  return y;
}
__device__ __forceinline__ float shape_step(float s, float p, float ceiling, float release) {
#pragma clang fp contract(off)
  const float t = p > ceiling ? ceiling / p : 1.0f;
  float u = 1.0f - s;
  u = release * u;
  const float r = s + u;
  return t < r ? t : r;
}
__global__ __launch_bounds__(256) void shape_kernel(const uint32_t* __restrict__ tab, uint32_t* __restrict__ state, int64_t state_pitch,
                                                    const float* __restrict__ ramps, float* __restrict__ out_peak,
                                                    float* __restrict__ out_gain, int64_t out_pitch) {
  __shared__ float tile[kShapeTile];
  __shared__ float bpk[kShapePassBlocks + 1], bn[kShapePassBlocks + 2];
  __shared__ uint32_t seg[kShapeMaxSegs * kShapeSegWords];
  __shared__ float red_in[4], red_out[4], sh_c;
  __shared__ int red_clamped[4], sh_leave;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* row = tab + (size_t)s * kShapeWords;
  const int n_new = (int)row[4], flags = (int)row[6];
  const bool final = flags & 1, limit = flags & 2;
  if (n_new <= 0 && !final) return;                     // idle (uniform: in front of the first barrier)
  float* dst = reinterpret_cast<float*>(((uint64_t)row[1] << 32) | row[0]);
  const float* src = reinterpret_cast<const float*>(((uint64_t)row[3] << 32) | row[2]);
  const int hold = (int)row[5], N = (int)row[7], nseg = (int)row[12];
  const float ceiling = __uint_as_float(row[8]), release = __uint_as_float(row[9]), rN = __uint_as_float(row[10]);
  const float base = __uint_as_float(row[11]);
  if (tid < kShapeMaxSegs * kShapeSegWords) seg[tid] = row[kShapeSegBase + tid];
  if (tid == 0) sh_c = 0.0f;
  uint32_t* srow = state + (size_t)s * state_pitch;
  float* held = reinterpret_cast<float*>(srow + kShapeHeader);
  // the recursion's state: thread 0 alone advances it
  const bool fresh = (int)srow[5] == 0;
  float sl = fresh ? 1.0f : __uint_as_float(srow[0]), node = fresh ? 1.0f : __uint_as_float(srow[1]);
  float s_min = fresh ? 1.0f : __uint_as_float(srow[8]), open_peak = 0.0f;
  int blocks = (int)srow[4], limited = (int)srow[9], n_blk = 0;
  float* opk = out_peak + (int64_t)s * out_pitch;
  float* ogn = out_gain + (int64_t)s * out_pitch;
  const int M = hold + n_new;                           // the local stream
  const int nb_all = (M + N - 1) / N, PB = min(kShapePassBlocks, kShapePassSamples / N), ov = limit ? 1 : 0;
  float my_in = 0.0f, my_out = 0.0f;
  int my_clamped = 0, n_out = 0, n_hold = 0;
  __syncthreads();                                      // seg, sh_c
  for (int b0 = 0; b0 < nb_all; b0 += PB) {
    const bool last = b0 + PB + ov >= nb_all;
    const int nt = min(PB + ov, nb_all - b0);           // blocks in the tile
    const int T0 = b0 * N, hiq = min(nt * N, M - T0);   // tile[q] is local position T0 + q; q in [0, hiq) exists
    // (a) the held samples, then the new ones as v = z * c
    const int nh = max(0, min(hiq, hold - T0));
    for (int q = tid; q < nh; q += 256) tile[q] = held[T0 + q];
    {
      const int i0 = T0 + nh - hold, cnt = hiq - nh;    // new samples [i0, i0 + cnt) of the launch go to tile[nh ...]
      const float* g = src + i0;
      float* t = tile + nh;
      const int head = min(cnt, (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u));
      const int nv = (cnt - head) >> 2, tail0 = head + 4 * nv;
      auto take = [&](int e, float z) {
        const float c = shape_gain(seg, nseg, base, ramps, i0 + e);
        my_in = fmaxf(my_in, fabsf(z));
        if (i0 + e == n_new - 1) sh_c = c;
        t[e] = z * c;
      };
      if (tid < head) take(tid, g[tid]);
      for (int v = tid; v < nv; v += 256) {
        const int e = head + 4 * v;
        const float4 x = *reinterpret_cast<const float4*>(g + e);
        take(e, x.x); take(e + 1, x.y); take(e + 2, x.z); take(e + 3, x.w);
      }
      if (tid < cnt - tail0) take(tail0 + tid, g[tail0 + tid]);
    }
    __syncthreads();
    if (limit) {
      // (b) the peak of every block of the tile
      for (int j = wave; j < nt; j += 4) {              // wave-uniform
        const int a = j * N, z = min(hiq, (j + 1) * N);
        float m = 0.0f;
        for (int q = a + lane; q < z; q += 64) m = fmaxf(m, fabsf(tile[q]));
        for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) bpk[j] = m;
      }
      __syncthreads();
      // (c) the recursion, in block order
      if (tid == 0) {
        int nc = 0;                                     // blocks of the tile whose start node is known: a prefix
        for (int j = 0; j < nt; ++j) {
          if (j == 0 && (b0 > 0 || hold >= N)) {        // completed by an earlier pass or an earlier launch
            bn[0] = node;
            nc = 1;
            continue;
          }
          const float p = bpk[j];
          if (min(hiq, (j + 1) * N) - j * N < N && !final) { open_peak = p; break; }          // the block the launch leaves open
          const float sb = shape_step(sl, p, ceiling, release);
          bn[j] = sl < sb ? sl : sb;
          sl = sb;
          s_min = s_min < sb ? s_min : sb;
          limited += p > ceiling ? 1 : 0;
          blocks += 1;
          opk[n_blk] = p; ogn[n_blk] = sb;
          ++n_blk;
          nc = j + 1;
        }
        int leave;
        if (last && final) { bn[nc] = sl; leave = nc; }
        else leave = max(0, nc - 1);
        if (!last) node = bn[PB];
        else node = leave < nc ? bn[nc - 1] : sl;
        sh_leave = leave;
      }
      __syncthreads();
    }
    // (d) ramp, gain and clamp, from the tile to dst on its own 16-byte grid
    const int leave = limit ? sh_leave : nt;
    const int hi = min(leave * N, hiq);
    {
      float* g = dst + T0;
      const int head = min(hi, (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u));
      const int nv = (hi - head) >> 2, tail0 = head + 4 * nv;
      auto one = [&](int q) {
        const int j = q / N;
        return shape_apply(tile[q], limit ? bn[j] : 1.0f, limit ? bn[j + 1] : 1.0f, q - j * N, rN, ceiling, my_out, my_clamped);
      };
      if (tid < head) g[tid] = one(tid);
      for (int v = tid; v < nv; v += 256) {
        const int q = head + 4 * v;
        const float y0 = one(q), y1 = one(q + 1), y2 = one(q + 2), y3 = one(q + 3);
        *reinterpret_cast<float4*>(g + q) = make_float4(y0, y1, y2, y3);
      }
      if (tid < hi - tail0) g[tail0 + tid] = one(tail0 + tid);
    }
    if (last) {
      n_out = T0 + hi;
      n_hold = hiq - hi;
      // (e) what did not leave goes back to the row
      if (limit) {
        for (int q = tid; q < n_hold; q += 256) held[q] = tile[hi + q];
      }
    }
    __syncthreads();                                    // the next pass overwrites the tile and the nodes
    if (last) break;                                    // uniform: the pass that held every block to the end of the stream
  }
  if (limit)
    for (int q = n_hold + tid; q < 2 * N - 1; q += 256) held[q] = 0.0f;
  for (int o = 32; o; o >>= 1) {
    my_in = fmaxf(my_in, __shfl_xor(my_in, o));
    my_out = fmaxf(my_out, __shfl_xor(my_out, o));
    my_clamped += __shfl_xor(my_clamped, o);
  }
  if (lane == 0) { red_in[wave] = my_in; red_out[wave] = my_out; red_clamped[wave] = my_clamped; }
  __syncthreads();
  if (tid == 0) {
    const float pin = fmaxf(fmaxf(red_in[0], red_in[1]), fmaxf(red_in[2], red_in[3]));
    const float pout = fmaxf(fmaxf(red_out[0], red_out[1]), fmaxf(red_out[2], red_out[3]));
    const int cl = red_clamped[0] + red_clamped[1] + red_clamped[2] + red_clamped[3];
    srow[0] = __float_as_uint(sl); srow[1] = __float_as_uint(node); srow[2] = __float_as_uint(open_peak);
    srow[3] = (uint32_t)n_hold; srow[4] = (uint32_t)blocks; srow[5] = (uint32_t)((int)srow[5] + n_new);
    srow[6] = (uint32_t)((int)srow[6] + n_out);
    if (n_new > 0) srow[7] = __float_as_uint(sh_c);
    srow[8] = __float_as_uint(s_min); srow[9] = (uint32_t)limited; srow[10] = (uint32_t)((int)srow[10] + cl);
    srow[11] = __float_as_uint(fmaxf(__uint_as_float(srow[11]), pin));
    srow[12] = __float_as_uint(fmaxf(__uint_as_float(srow[12]), pout));
  }
}

}  // namespace dmel

extern "C" int dmel_shape_items(float* const* dst, const int64_t* dst_cap, const float* const* src, const int64_t* n_new,
                                const int64_t* hold, const int32_t* flags, const int32_t* N, const float* fparams,
                                const int32_t* seg_count, const int32_t* segs, int S, const float* ramps, int64_t ramp_floats, void* state,
                                int64_t state_pitch, float* out_peak, float* out_gain, int64_t out_pitch, void* table_scratch,
                                void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(dst && dst_cap && src && n_new && hold && flags && N && fparams && seg_count && segs && state && out_peak && out_gain &&
                     table_scratch,
                 "shape_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "shape_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG(ramp_floats >= 0 && (ramps || ramp_floats == 0), "shape_items: a ramp arena of %lld floats (NULL: %d)",
                 (long long)ramp_floats, (int)!ramps);
  DMEL_CHECK_ARG((((uintptr_t)state | (uintptr_t)out_peak | (uintptr_t)out_gain | (uintptr_t)ramps) & 3) == 0,
                 "shape_items: state, out_peak, out_gain or ramps is not 4-byte aligned");
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 7) == 0, "shape_items: table_scratch is not 8-byte aligned");
  DMEL_CHECK_ARG(state_pitch >= kShapeHeader && out_pitch >= 0, "shape_items: a state pitch of %lld words (at least %d) or a negative "
                 "output pitch %lld", (long long)state_pitch, kShapeHeader, (long long)out_pitch);
  static const char* const kNames[kShapeFparams] = {"ceiling", "release", "rN", "base gain", "max_gain"};
  std::vector<uint32_t> tab((size_t)kShapeWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s];
    DMEL_CHECK_ARG(n >= 0 && n <= 0x3fffffff, "shape_items: item %d: %lld new samples, expected 0 .. 2^30 - 1", s, (long long)n);
    DMEL_CHECK_ARG(flags[s] >= 0 && flags[s] <= 3, "shape_items: item %d: flags %d, expected 0 .. 3 (1: final, 2: limit)", s, flags[s]);
    const bool fin = flags[s] & 1, lim = flags[s] & 2;
    if (n == 0 && !fin) continue;                       // idle: its parameters are not looked at (the table row stays 0)
    int32_t nb = N[s];
    int64_t leave = n, done = 0;
    if (lim) {
      DMEL_CHECK_ARG(nb >= kShapeMinBlock && nb <= kShapeMaxBlock, "shape_items: item %d: a block of %d samples, expected %d .. %d", s, nb,
                     kShapeMinBlock, kShapeMaxBlock);
      DMEL_CHECK_ARG(hold[s] >= 0 && hold[s] <= 2 * (int64_t)nb - 1, "shape_items: item %d: %lld held samples, expected 0 .. 2 N - 1 = %d", s,
                     (long long)hold[s], 2 * nb - 1);
      DMEL_CHECK_ARG(state_pitch >= kShapeHeader + 2 * (int64_t)nb - 1, "shape_items: item %d: a state row of %lld words, a block of %d "
                     "needs %d", s, (long long)state_pitch, nb, kShapeHeader + 2 * nb - 1);
      const int64_t total = hold[s] + n;
      leave = fin ? total : std::max<int64_t>(0, total / nb - 1) * nb;
      done = total / nb + (fin && total % nb ? 1 : 0) - (hold[s] >= nb ? 1 : 0);
      DMEL_CHECK_ARG(out_pitch >= done, "shape_items: item %d: the step completes %lld blocks, which exceed the output pitch %lld", s,
                     (long long)done, (long long)out_pitch);
    } else {
      DMEL_CHECK_ARG(hold[s] == 0, "shape_items: item %d: %lld held samples without the limiter", s, (long long)hold[s]);
      nb = kShapeMaxBlock;                              // the tile's grid; no block of the rule
    }
    DMEL_CHECK_ARG(dst_cap[s] >= leave, "shape_items: item %d: the step hands out %lld samples, its destination takes %lld", s,
                   (long long)leave, (long long)dst_cap[s]);
    DMEL_CHECK_ARG((dst[s] || leave == 0) && (src[s] || n == 0), "shape_items: item %d: NULL %s", s, src[s] || n == 0 ? "destination" : "source");
    DMEL_CHECK_ARG((((uintptr_t)dst[s] | (uintptr_t)src[s]) & 3) == 0, "shape_items: item %d: a pointer is not 4-byte aligned", s);
    const float* fp = fparams + (size_t)kShapeFparams * s;
    for (int k = 0; k < kShapeFparams; ++k)             // the base gain alone may be 0
      DMEL_CHECK_ARG(std::isfinite(fp[k]) && (fp[k] > 0.0f || (k == 3 && fp[k] == 0.0f)),
                     "shape_items: item %d: float parameter %d (%s) is not finite and positive", s, k, kNames[k]);
    DMEL_CHECK_ARG(fp[1] <= 1.0f && fp[2] <= 1.0f, "shape_items: item %d: release %g or rN %g above 1", s, (double)fp[1], (double)fp[2]);
    DMEL_CHECK_ARG(fp[3] <= fp[4], "shape_items: item %d: base gain %g above max_gain %g", s, (double)fp[3], (double)fp[4]);
    const int32_t count = seg_count[s];
    DMEL_CHECK_ARG(count >= 0 && count <= kShapeMaxSegs, "shape_items: item %d: %d live segments, expected 0 .. %d", s, count, kShapeMaxSegs);
    uint32_t* it = tab.data() + (size_t)kShapeWords * s;
    int32_t before = INT32_MIN;
    for (int k = 0; k < count; ++k) {
      const int32_t* w = segs + ((size_t)kShapeMaxSegs * s + k) * kShapeSegWords;
      float g[2];
      std::memcpy(g, w + 3, sizeof g);
      DMEL_CHECK_ARG(w[0] >= -(1 << 30) && w[0] <= (1 << 30) && w[0] >= before,
                     "shape_items: item %d: segment %d: start %d, expected -2^30 .. 2^30 and no decrease", s, k, w[0]);
      DMEL_CHECK_ARG(w[1] >= 0 && w[1] <= kShapeMaxRamp, "shape_items: item %d: segment %d: ramp = %d, expected 0 .. %d", s, k, w[1],
                     kShapeMaxRamp);
      DMEL_CHECK_ARG(w[1] == 0 || (w[2] >= 0 && (int64_t)w[2] + w[1] <= ramp_floats),
                     "shape_items: item %d: segment %d: ramp table [%d, %d + %d) lies beyond the arena of %lld floats", s, k, w[2], w[2],
                     w[1], (long long)ramp_floats);
      for (int j = 0; j < 2; ++j)
        DMEL_CHECK_ARG(std::isfinite(g[j]) && g[j] >= 0.0f && g[j] <= fp[4],
                       "shape_items: item %d: segment %d: g%d = %g, expected a finite gain in [0, max_gain = %g]", s, k, j, (double)g[j],
                       (double)fp[4]);
      before = w[0];
      std::memcpy(it + kShapeSegBase + (size_t)kShapeSegWords * k, w, kShapeSegWords * sizeof(int32_t));
    }
    const uint64_t d = (uint64_t)(uintptr_t)dst[s], x = (uint64_t)(uintptr_t)src[s];
    it[0] = (uint32_t)d; it[1] = (uint32_t)(d >> 32); it[2] = (uint32_t)x; it[3] = (uint32_t)(x >> 32);
    it[4] = (uint32_t)n; it[5] = (uint32_t)hold[s]; it[6] = (uint32_t)flags[s]; it[7] = (uint32_t)nb;
    std::memcpy(it + 8, fp, 4 * sizeof(float));
    it[12] = (uint32_t)count;
    ++live;
    bytes += 4.0 * (double)n + 4.0 * (double)leave + 8.0 * (double)done + 8.0 * kShapeHeader + (lim ? 8.0 * (2.0 * nb - 1.0) : 0.0);
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per shape launch (dmel_prof_read("shape"))
    ProfScope ps("small", st, 0.0, bytes), count("shape", st, 0.0, 0.0);
    hipLaunchKernelGGL(shape_kernel, dim3((unsigned)S), dim3(256), 0, st, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), state_pitch, ramps, out_peak, out_gain, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

namespace dmel {

// ---- speaking rate on codec-rate audio (include/dmel_hip.h: dmel_pace_items; the rule and the state row: utils/pace.py) ----------------
// Row s of the table is 64 4-byte words: dst (2), src (2), n_new, hold, flags (1: final), H, D, floor, eps, K, a_{K-1}, a_K, fed, the
// frames the step completes, the samples it hands out, the base rate, the request count, the offset of the weight table, zeros, and
// from word 32 eight request records of two words (position relative to the first new sample, permille); workgroup s owns slot s.
// The slot's stream x is addressed by ABSOLUTE positions: [fed - hold, fed) are the held samples of its state row, [fed, fed + n_new)
// the new ones, 0.0 behind them.  A WINDOW of 6144 consecutive positions sits in LDS; a frame needs [min(t, a - D), max(t, a + D) + H),
// at most 2 H + 2 D = 2048 positions, and the window is re-filled from the frame's lowest position when that range leaves it.  The
// frames of a slot run in order: (a) the natural-continuation test on uniform integers; (b) otherwise the work items are (candidate,
// sum8 segment) pairs, candidates in passes of 511, the template's own energy riding as one more candidate of the first pass: item
// c is segment c / cnt, candidate c % cnt, so the lanes of a wave read consecutive window words (conflict-free) and the same template
// word (a broadcast), each item one sequential sum of H / 8 terms; (c) thread c joins the eight partial sums of candidate c by the
// fixed tree, forms q and keeps its best (q, |d|, d) key; the keys meet by wave shuffles and one LDS round -- the order is total, so
// any reduction order gives the same winner; (d) thread i blends sample i and stores it.  Behind the last frame the window is
// re-filled from the position the rule keeps from, and that part goes back to the row.  Every operation of the rule is rounded on
// its own (fp contract(off)).  Plain stores, no atomics.
constexpr int kPaceWords = 64, kPaceHeader = 16, kPaceMinHop = 64, kPaceMaxHop = 512, kPaceMaxSearch = 512, kPaceWindow = 6144;
constexpr int kPacePass = 511, kPaceStride = kPacePass + 1, kPaceThreads = 512, kPaceMaxReq = 8, kPaceReqBase = 32;
constexpr int kPaceMinRate = 500, kPaceMaxRate = 2000, kPaceMaxNew = 1 << 26;
__host__ __device__ __forceinline__ int pace_rate_at(const int32_t* req, int nreq, int base, int64_t rel) {
  int r = base;
  for (int q = 0; q < nreq; ++q)
    if ((int64_t)req[2 * q] <= rel) r = req[2 * q + 1];   // positions do not decrease: the last one at or in front of rel
  return r;
}
__host__ __device__ __forceinline__ int pace_hop(int H, int permille) { return (H * permille + 500) / 1000; }
// (q, d) beats (oq, od): the larger value, then the smaller |d|, then the negative d
__device__ __forceinline__ bool pace_better(float q, int d, float oq, int od) {
  const int a = d < 0 ? -d : d, oa = od < 0 ? -od : od;
  return q > oq || (q == oq && (a < oa || (a == oa && d < od)));
}
__global__ __launch_bounds__(kPaceThreads) void pace_kernel(const uint32_t* __restrict__ tab, uint32_t* __restrict__ state,
                                                            int64_t state_pitch, const float* __restrict__ weights,
                                                            int32_t* __restrict__ out_offset, float* __restrict__ out_score,
                                                            int64_t out_pitch) {
#pragma clang fp contract(off)
  __shared__ float win[kPaceWindow];
  __shared__ float pc[8 * kPaceStride], pe[8 * kPaceStride];
  __shared__ float red_q[kPaceThreads / 64], sh_e0;
  __shared__ int red_d[kPaceThreads / 64];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* row = tab + (size_t)s * kPaceWords;
  const int n_new = (int)row[4], flags = (int)row[6];
  const bool final = flags & 1;
  if (n_new <= 0 && !final) return;                     // idle (uniform: in front of the first barrier)
  float* dst = reinterpret_cast<float*>(((uint64_t)row[1] << 32) | row[0]);
  const float* src = reinterpret_cast<const float*>(((uint64_t)row[3] << 32) | row[2]);
  const int hold = (int)row[5], H = (int)row[7], D = (int)row[8], h8 = H >> 3;
  const float floor_e = __uint_as_float(row[9]), eps = __uint_as_float(row[10]);
  int K = (int)row[11], a_prev = (int)row[12], a_next = (int)row[13];
  const int fed = (int)row[14], frames = (int)row[15], n_out = (int)row[16], base_rate = (int)row[17], nreq = (int)row[18];
  const float* W = weights + (int)row[19];
  const int32_t* req = reinterpret_cast<const int32_t*>(row + kPaceReqBase);
  uint32_t* srow = state + (size_t)s * state_pitch;
  float* held = reinterpret_cast<float*>(srow + kPaceHeader);
  const int sbase = fed - hold, L = fed + n_new;        // the stream has [sbase, L); 0.0 behind L
  // a row the rule made has |p_{K-1} - a_{K-1}| <= D; the clamp keeps any other row's reads inside the window
  int p_prev = K > 0 ? max(0, min(max((int)srow[1], a_prev - D), a_prev + D)) : 0;
  int natural = (int)srow[6], searched = (int)srow[7], quiet = (int)srow[8], permille = (int)srow[12];
  int last_off = (int)srow[10];
  float last_q = __uint_as_float(srow[11]);
  int32_t* ooff = out_offset + (int64_t)s * out_pitch;
  float* osc = out_score + (int64_t)s * out_pitch;
  auto fill = [&](int wb) {                             // win[q] = x[wb + q]
    for (int q = tid; q < kPaceWindow; q += kPaceThreads) {
      const int pos = wb + q;
      float v = 0.0f;
      if (pos >= fed) { if (pos < L) v = src[pos - fed]; }
      else if (pos >= sbase) v = held[pos - sbase];
      win[q] = v;
    }
  };
  int wb = 0;
  bool have = false;
  for (int j = 0; j < frames; ++j) {
    const int a = a_next, t = p_prev + H;
    const bool nat = K == 0 || (a - D <= t && t <= a + D);
    const int first = K == 0 ? 0 : t;                   // frame 0 reads x[0 : H]
    const int lo = nat ? first : min(t, max(0, a - D)), hi = (nat ? first : max(t, a + D)) + H;
    if (!have || lo < wb || hi > wb + kPaceWindow) {    // uniform
      __syncthreads();                                  // the frame before has read the window
      fill(lo);
      wb = lo; have = true;
      __syncthreads();
    }
    int p = first;
    float q = 0.0f;
    if (nat) natural += 1;
    else {
      const float* T = win + (t - wb);
      const int dlo = max(-D, -a), nc = D - dlo + 1;    // candidates d = dlo .. D
      float bq = -1.0f;
      int bd = 0x7fffffff;
      for (int c0 = 0; c0 < nc; c0 += kPacePass) {
        const int real = min(kPacePass, nc - c0), cnt = real + (c0 == 0 ? 1 : 0);      // + the template against itself
        for (int c = tid; c < cnt * 8; c += kPaceThreads) {
          const int seg = c / cnt, ci = c - seg * cnt;
          const float* tp = T + seg * h8;
          const float* bp = ci < real ? win + (a + dlo + c0 + ci - wb) + seg * h8 : tp;
          float ac = 0.0f, ae = 0.0f;
          for (int i = 0; i < h8; ++i) {
            const float tv = tp[i], bv = bp[i];
            const float tb = tv * bv;
            ac = ac + tb;
            const float bb = bv * bv;
            ae = ae + bb;
          }
          pc[seg * kPaceStride + ci] = ac;
          pe[seg * kPaceStride + ci] = ae;
        }
        __syncthreads();
        if (tid < cnt) {
          float sc[8], se[8];
#pragma unroll
          for (int g = 0; g < 8; ++g) { sc[g] = pc[g * kPaceStride + tid]; se[g] = pe[g * kPaceStride + tid]; }
          const float cc = echo_tree(sc), e = echo_tree(se);
          if (tid < real) {
            float qv = 0.0f;
            if (cc > 0.0f) {
              const float c2 = cc * cc;
              const float ee = e + eps;
              qv = c2 / ee;
            }
            const int d = dlo + c0 + tid;
            if (pace_better(qv, d, bq, bd)) { bq = qv; bd = d; }
          } else sh_e0 = e;
        }
        __syncthreads();                                // the next pass overwrites the partial sums
      }
      for (int o = 32; o; o >>= 1) {
        const float oq = __shfl_xor(bq, o);
        const int od = __shfl_xor(bd, o);
        if (pace_better(oq, od, bq, bd)) { bq = oq; bd = od; }
      }
      if (lane == 0) { red_q[wave] = bq; red_d[wave] = bd; }
      __syncthreads();
      bq = red_q[0]; bd = red_d[0];
      for (int w = 1; w < kPaceThreads / 64; ++w)
        if (pace_better(red_q[w], red_d[w], bq, bd)) { bq = red_q[w]; bd = red_d[w]; }
      if (sh_e0 < floor_e) { p = a; quiet += 1; }
      else { p = a + bd; q = bq; searched += 1; }
    }
    const int emit = min(H, n_out - j * H);
    if (tid < emit) {
      const float old = win[first - wb + tid];
      float y = old;
      if (p != first) {
        float m = win[p - wb + tid] - old;
        m = W[tid] * m;
        y = old + m;
      }
      dst[(int64_t)j * H + tid] = y;
    }
    if (tid == 0) { ooff[j] = p - a; osc[j] = q; }
    last_off = p - a; last_q = q;
    permille = pace_rate_at(req, nreq, base_rate, (int64_t)a - fed);
    a_prev = a; a_next = a + pace_hop(H, permille);
    p_prev = p; K += 1;
  }
  // what the rule keeps goes back to the row
  const int cap = 2 * H + 2 * D;
  int keep = final ? L : (K == 0 ? 0 : min(L, max(0, min(a_prev + H, a_next) - D)));
  keep = max(keep, max(sbase, L - (cap - 1)));           // no-ops for integers the rule made
  const int n_hold = L - keep;
  __syncthreads();                                      // the last frame has read the window, and red_q / sh_e0
  fill(keep);
  __syncthreads();
  for (int q = tid; q < cap; q += kPaceThreads) held[q] = q < n_hold ? win[q] : 0.0f;
  if (tid == 0) {
    srow[0] = (uint32_t)K; srow[1] = (uint32_t)p_prev; srow[2] = (uint32_t)a_prev; srow[3] = (uint32_t)a_next;
    srow[4] = (uint32_t)L; srow[5] = (uint32_t)n_hold; srow[6] = (uint32_t)natural; srow[7] = (uint32_t)searched;
    srow[8] = (uint32_t)quiet; srow[9] = (uint32_t)((int)srow[9] + n_out); srow[10] = (uint32_t)last_off;
    srow[11] = __float_as_uint(last_q); srow[12] = (uint32_t)permille;
  }
}

}  // namespace dmel

extern "C" int dmel_pace_items(float* const* dst, const int64_t* dst_cap, const float* const* src, const int64_t* n_new,
                               const int64_t* ints, const int32_t* flags, const int32_t* H, const int32_t* D, const float* fparams,
                               const int32_t* base_permille, const int32_t* req_count, const int32_t* reqs, int S, const float* weights,
                               int64_t weight_floats, const int32_t* weight_off, void* state, int64_t state_pitch, int32_t* out_offset,
                               float* out_score, int64_t out_pitch, void* table_scratch, void* stream) {
  using namespace dmel;
  DMEL_CHECK_ARG(dst && dst_cap && src && n_new && ints && flags && H && D && fparams && base_permille && req_count && reqs && weights &&
                     weight_off && state && out_offset && out_score && table_scratch,
                 "pace_items: NULL argument");
  DMEL_CHECK_ARG(S >= 1 && S <= 65535, "pace_items: %d items, expected 1 .. 65535", S);
  DMEL_CHECK_ARG(weight_floats >= 0, "pace_items: a weight arena of %lld floats", (long long)weight_floats);
  DMEL_CHECK_ARG((((uintptr_t)state | (uintptr_t)out_offset | (uintptr_t)out_score | (uintptr_t)weights) & 3) == 0,
                 "pace_items: state, out_offset, out_score or weights is not 4-byte aligned");
  DMEL_CHECK_ARG(((uintptr_t)table_scratch & 7) == 0, "pace_items: table_scratch is not 8-byte aligned");
  DMEL_CHECK_ARG(state_pitch >= kPaceHeader && out_pitch >= 0, "pace_items: a state pitch of %lld words (at least %d) or a negative "
                 "output pitch %lld", (long long)state_pitch, kPaceHeader, (long long)out_pitch);
  std::vector<uint32_t> tab((size_t)kPaceWords * S, 0u);
  int64_t live = 0;
  double bytes = 0.0;
  for (int s = 0; s < S; ++s) {
    const int64_t n = n_new[s];
    DMEL_CHECK_ARG(n >= 0 && n <= kPaceMaxNew, "pace_items: item %d: %lld new samples, expected 0 .. 2^26", s, (long long)n);
    DMEL_CHECK_ARG(flags[s] >= 0 && flags[s] <= 1, "pace_items: item %d: flags %d, expected 0 .. 1 (1: final)", s, flags[s]);
    const bool fin = flags[s] & 1;
    if (n == 0 && !fin) continue;                       // idle: its parameters are not looked at (the table row stays 0)
    const int32_t h = H[s], d = D[s];
    DMEL_CHECK_ARG(h >= kPaceMinHop && h <= kPaceMaxHop && h % 8 == 0, "pace_items: item %d: a hop of %d samples, expected a multiple of 8 "
                   "in %d .. %d", s, h, kPaceMinHop, kPaceMaxHop);
    DMEL_CHECK_ARG(d >= 0 && d <= kPaceMaxSearch, "pace_items: item %d: a search half-width of %d samples, expected 0 .. %d", s, d,
                   kPaceMaxSearch);
    const int64_t* iv = ints + (size_t)5 * s;
    const int64_t K0 = iv[0], ap0 = iv[1], an0 = iv[2], fed = iv[3], hold = iv[4];
    DMEL_CHECK_ARG(hold >= 0 && hold < 2 * (int64_t)h + 2 * d, "pace_items: item %d: %lld held samples, expected 0 .. 2 H + 2 D - 1 = %d", s,
                   (long long)hold, 2 * h + 2 * d - 1);
    DMEL_CHECK_ARG(state_pitch >= kPaceHeader + 2 * (int64_t)h + 2 * d, "pace_items: item %d: a state row of %lld words, H = %d and D = %d "
                   "need %d", s, (long long)state_pitch, h, d, kPaceHeader + 2 * h + 2 * d);
    DMEL_CHECK_ARG(fed >= hold && fed <= ((int64_t)1 << 30), "pace_items: item %d: %lld samples fed, expected the %lld held .. 2^30", s,
                   (long long)fed, (long long)hold);
    DMEL_CHECK_ARG(K0 >= 0 && K0 < ((int64_t)1 << 30) && ap0 >= 0 && (K0 == 0 ? an0 == 0 && ap0 == 0
                                                                              : an0 - ap0 >= h / 2 && an0 - ap0 <= 2 * h && an0 <= fed + 2 * h),
                   "pace_items: item %d: the integers K = %lld, a_{K-1} = %lld, a_K = %lld are none the rule makes with %lld samples fed", s,
                   (long long)K0, (long long)ap0, (long long)an0, (long long)fed);
    DMEL_CHECK_ARG((((uintptr_t)dst[s] | (uintptr_t)src[s]) & 3) == 0, "pace_items: item %d: a pointer is not 4-byte aligned", s);
    const float* fp = fparams + (size_t)2 * s;
    DMEL_CHECK_ARG(std::isfinite(fp[0]) && fp[0] >= 0.0f && std::isfinite(fp[1]) && fp[1] > 0.0f,
                   "pace_items: item %d: floor %g is not finite or is negative, or eps %g is not finite and positive", s, (double)fp[0],
                   (double)fp[1]);
    const int32_t base = base_permille[s], count = req_count[s];
    DMEL_CHECK_ARG(base >= kPaceMinRate && base <= kPaceMaxRate, "pace_items: item %d: a rate of %d permille, expected %d .. %d", s, base,
                   kPaceMinRate, kPaceMaxRate);
    DMEL_CHECK_ARG(count >= 0 && count <= kPaceMaxReq, "pace_items: item %d: %d live requests, expected 0 .. %d", s, count, kPaceMaxReq);
    const int32_t* rq = reqs + (size_t)2 * kPaceMaxReq * s;
    int32_t before = INT32_MIN;
    for (int k = 0; k < count; ++k) {
      DMEL_CHECK_ARG(rq[2 * k] >= -(1 << 30) && rq[2 * k] <= (1 << 30) && rq[2 * k] >= before,
                     "pace_items: item %d: request %d: position %d, expected -2^30 .. 2^30 and no decrease", s, k, rq[2 * k]);
      DMEL_CHECK_ARG(rq[2 * k + 1] >= kPaceMinRate && rq[2 * k + 1] <= kPaceMaxRate,
                     "pace_items: item %d: request %d: a rate of %d permille, expected %d .. %d", s, k, rq[2 * k + 1], kPaceMinRate,
                     kPaceMaxRate);
      before = rq[2 * k];
    }
    DMEL_CHECK_ARG(weight_off[s] >= 0 && (int64_t)weight_off[s] + h <= weight_floats,
                   "pace_items: item %d: weight table [%d, %d + %d) lies beyond the arena of %lld floats", s, weight_off[s], weight_off[s], h,
                   (long long)weight_floats);
    // the step on integers, as utils/pace.py: advance
    const int64_t L = fed + n;
    int64_t K = K0, ap = ap0, an = an0, fr = 0;
    while (fin ? an < L : L >= (K == 0 ? (int64_t)h : std::max(ap + 2 * h, an + h) + d)) {
      const int r = pace_rate_at(rq, count, base, an - fed);
      ap = an; an += pace_hop(h, r);
      ++K; ++fr;
    }
    int64_t leave = fr * h;
    if (fin && fr) leave -= h - std::min<int64_t>(h, L - ap);
    DMEL_CHECK_ARG(out_pitch >= fr, "pace_items: item %d: the step completes %lld frames, which exceed the output pitch %lld", s,
                   (long long)fr, (long long)out_pitch);
    DMEL_CHECK_ARG(dst_cap[s] >= leave, "pace_items: item %d: the step hands out %lld samples, its destination takes %lld", s,
                   (long long)leave, (long long)dst_cap[s]);
    DMEL_CHECK_ARG((dst[s] || leave == 0) && (src[s] || n == 0), "pace_items: item %d: NULL %s", s, src[s] || n == 0 ? "destination" : "source");
    uint32_t* it = tab.data() + (size_t)kPaceWords * s;
    const uint64_t dp = (uint64_t)(uintptr_t)dst[s], xp = (uint64_t)(uintptr_t)src[s];
    it[0] = (uint32_t)dp; it[1] = (uint32_t)(dp >> 32); it[2] = (uint32_t)xp; it[3] = (uint32_t)(xp >> 32);
    it[4] = (uint32_t)n; it[5] = (uint32_t)hold; it[6] = (uint32_t)flags[s]; it[7] = (uint32_t)h; it[8] = (uint32_t)d;
    std::memcpy(it + 9, fp, 2 * sizeof(float));
    it[11] = (uint32_t)K0; it[12] = (uint32_t)ap0; it[13] = (uint32_t)an0; it[14] = (uint32_t)fed; it[15] = (uint32_t)fr;
    it[16] = (uint32_t)leave; it[17] = (uint32_t)base; it[18] = (uint32_t)count; it[19] = (uint32_t)weight_off[s];
    std::memcpy(it + kPaceReqBase, rq, (size_t)2 * count * sizeof(int32_t));
    ++live;
    bytes += 4.0 * (double)n + 4.0 * (double)leave + 8.0 * (double)fr + 8.0 * kPaceHeader + 4.0 * (double)hold + 4.0 * (2.0 * h + 2.0 * d);
  }
  if (live == 0) return DMEL_OK;                        // every item idle
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(launch_table_put(tab.data(), tab.size() * sizeof(uint32_t), table_scratch, st));
  {
    // "small" carries the time and the bytes; the second scope only counts: one record per pace launch (dmel_prof_read("pace"))
    ProfScope ps("small", st, 0.0, bytes), count("pace", st, 0.0, 0.0);
    hipLaunchKernelGGL(pace_kernel, dim3((unsigned)S), dim3(kPaceThreads), 0, st, static_cast<const uint32_t*>(table_scratch),
                       static_cast<uint32_t*>(state), state_pitch, weights, out_offset, out_score, out_pitch);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}
