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
// One workgroup owns up to 3 x 1008 consecutive outputs of one (b, c) row: each tile's row segment (+6/+6 halo) is read from HBM once
// into LDS, the activated 2x signal lives only in LDS, and the store is coalesced.  HBM traffic = 1 read + 1 write per element, the
// algorithmic minimum (8 B/element); the reference kernel's stride-32-per-thread addressing is uncoalesced.
// Measured on the MI355X (profiles/aa_snake_blocked.txt), register-blocked form against the one-output-per-thread form it replaced, same
// bits: 51 against 86 vector instructions and 15.7 against 45.9 LDS-array cycles per 64 outputs (rocprofv3 --pmc, no bank conflicts in
// either), 3.9-4.6 against 3.0-3.7 TB/s on the 24 M-element benchmark tensors, 2.99 against 3.60 ms per benchmark step.  Both earlier
// notes in this file against this form are superseded: v_pk_fma_f32 (which the compiler emits for the neighbouring samples' FMA chains,
// about half of the kernel's vector instructions) does not issue at half rate, and four samples per thread, 0.84x when it was tried
// before the two-tile prefetch, is 1.2x with it.
#include "ops.h"
#include "snake_dev.h"

namespace dmel {

constexpr int kSnakeTile = 1024;        // the backward kernels' tile
constexpr int kSnakeFwdTile = 1008;     // the forward kernel's: 4 * 252 outputs, 1014 pairs, a 1020-sample row segment

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Register-blocked forward: every thread owns FOUR consecutive elements in each of the three stages of a tile, and every LDS access
// and (on aligned rows) every global access is 16 bytes wide.  For the tile that starts at output t0 (a multiple of 4):
//   xs[k] = x[clamp(t0 - 8 + k)], k = 0..1023     thread q fills xs[4q .. 4q+3]: one global_load_dwordx4 from x + t0 - 8 + 4q when the
//                                                 row is 16-byte aligned and T % 4 == 0 (VEC), one ds_write_b128
//   pair p <-> m = t0 - 3 + p, p = 0..len+5       thread q computes pairs 4q .. 4q+3 from the 10 samples x[m-3 .. m+3+3] = xs[4q+2 .. 4q+11]
//                                                 (xp[d] of the formulas above is xs[p + 5 + d]): three ds_read_b128 of xs[4q .. 4q+11]
//   ve[p], vo[p]: the activated 2x signal as two planes, written as one ds_write_b128 each at [4q .. 4q+3]
//   out[t0 + o] needs vo[o .. o+5], ve[o+1 .. o+6] thread r computes o = 4r .. 4r+3 from ve[4r+1 .. 4r+9], vo[4r .. 4r+8]: three
//                                                 ds_read_b128 of each plane at [4r .. 4r+11], one global_store_dwordx4 to y + t0 + 4r
// Alignment: xs, ve and vo are 16-byte aligned arrays of 1024 floats and every 16-byte LDS access above starts at float index 4q + {0, 4, 8}
// -- a multiple of 16 bytes by construction, whatever t0, len or T are.  The largest index touched is 4 * 253 + 11 = 1023 (pairs: 4q <=
// len + 5 <= 1013; outputs: 4r <= len - 1 <= 1007).  At a 16-byte lane stride ds_read_b128 is conflict-free (MI355X lane groups).
// Whole passes: 1008 outputs = 252 threads x 4, 1014 pairs = 254 threads x 4 (the last two of 1016 are computed and never read), and the
// 1020-sample segment t0-6 .. t0+1013 sits at k = 2..1021 of the 1024 floats that 256 threads x 4 load: one pass per stage, no straggler.
// The arithmetic of every element is the one of the formulas above in the same order, so where a tile or a row starts, and which of the
// two instantiations runs, never changes a bit.  Replicate padding of the 2x signal (pairs m < 0 and m > T-1) is patched into the planes by
// three threads between the stages, in the tiles that touch a row end only (block-uniform test).
// The tiles of ONE row: xr / yr point at column 0 of the (b, c) row, T is the number of valid columns of that row (its replicate padding
// ends at T - 1; nothing at or behind column T is read or written), `first` the first output of this workgroup's nsub tiles.
// The four stage bodies of a tile, shared by aa_snake_row, aa_snake3_row and snake_post_kernel: one expression per element, so every kernel
// built from them computes the same bits.
// this thread's four samples of the tile's row segment: xs[4 tid + i] = x[clamp(t0 - 8 + 4 tid + i, 0, T - 1)]
template <bool VEC>
__device__ __forceinline__ f32x4 snake_fetch4(const float* __restrict__ xr, int T, int t0, int tid) {
  const int s = t0 - 8 + 4 * tid;
  if (VEC && s >= 0 && s + 4 <= T) return *reinterpret_cast<const f32x4*>(xr + s);
  f32x4 v;
  v.x = xr[min(max(s, 0), T - 1)];
  v.y = xr[min(max(s + 1, 0), T - 1)];
  v.z = xr[min(max(s + 2, 0), T - 1)];
  v.w = xr[min(max(s + 3, 0), T - 1)];
  return v;
}
// pairs 4 tid .. 4 tid + 3 of the 2x signal BEFORE the snake: u[2 i] the even, u[2 i + 1] the odd sample of pair 4 tid + i
__device__ __forceinline__ void snake_up4(const float* xs, int tid, const Taps12& tu, float (&u)[8]) {
  float w[12];
  lds_read3_b128(xs + 4 * tid, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float ue = 0.f, uo = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      ue = fmaf(tu.f[2 * j + 1], w[i + 7 - j], ue);
      uo = fmaf(tu.f[2 * j], w[i + 8 - j], uo);
    }
    u[2 * i] = ue;
    u[2 * i + 1] = uo;
  }
}
// u <- snake(u) with one (a, 1 / b) for all eight, stored as the two planes
__device__ __forceinline__ void snake_store4(float (&u)[8], float a, float inv_b, float* ve, float* vo, int tid) {
  float aa[8], bb[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { aa[i] = a; bb[i] = inv_b; }
  // all eight sin^2 behind ONE wave-uniform test of the large-argument case, so the straight-line bodies interleave (snake_dev.h)
  snake_n(u, aa, bb);
  *reinterpret_cast<f32x4*>(ve + 4 * tid) = f32x4{u[0], u[2], u[4], u[6]};
  *reinterpret_cast<f32x4*>(vo + 4 * tid) = f32x4{u[1], u[3], u[5], u[7]};
}
// outputs 4 tid .. 4 tid + 3 of the tile from the two planes
__device__ __forceinline__ f32x4 snake_down4(const float* ve, const float* vo, int tid, const Taps12& td) {
  float e[12], o[12];
  lds_read3_b128(ve + 4 * tid, e);
  lds_read3_b128(vo + 4 * tid, o);
  f32x4 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float acc = td.f[0] * o[i];
#pragma unroll
    for (int k = 1; k < 6; ++k) {
      acc = fmaf(td.f[2 * k - 1], e[i + k], acc);
      acc = fmaf(td.f[2 * k], o[i + k], acc);
    }
    out[i] = fmaf(td.f[11], e[i + 6], acc);
  }
  return out;
}
// the effective (a, 1 / (b + 1e-9)) of channel c
__device__ __forceinline__ void snake_params(const float* __restrict__ alpha, const float* __restrict__ beta, int logscale, int c, float& a,
                                             float& inv_b) {
  a = alpha[c];
  float bt = beta ? beta[c] : a;
  if (logscale) {
    bt = beta ? expf(bt) : expf(a);
    a = expf(a);
  }
  inv_b = 1.0f / (bt + 1e-9f);
}

template <bool VEC>
__device__ __forceinline__ void aa_snake_row(const float* __restrict__ xr, float* __restrict__ yr, const float* __restrict__ alpha,
                                             const float* __restrict__ beta, const Taps12& tu, const Taps12& td, int logscale, int c, int T,
                                             int first, int nsub, float* xs, float* ve, float* vo) {
  float a, inv_b;
  snake_params(alpha, beta, logscale, c, a, inv_b);
  // nsub consecutive tiles per workgroup, SOFTWARE-PIPELINED: the row segment of tile s + 1 is fetched into registers before tile s is
  // computed.  A workgroup reads 4 KB and then computes for microseconds without touching memory; without the prefetch the bytes in
  // flight per CU, not instruction issue, set the read rate (Little's law).
  const int tid = threadIdx.x;
  f32x4 pre = {0.f, 0.f, 0.f, 0.f};
  if (first < T) pre = snake_fetch4<VEC>(xr, T, first, tid);
  for (int sub = 0; sub < nsub; ++sub) {
    const int t0 = first + sub * kSnakeFwdTile;
    if (t0 >= T) break;
    const int len = min(kSnakeFwdTile, T - t0);
    if (sub) __syncthreads();                  // the previous tile's reads of xs / ve / vo are done
    *reinterpret_cast<f32x4*>(xs + 4 * tid) = pre;
    if (sub + 1 < nsub && t0 + kSnakeFwdTile < T) pre = snake_fetch4<VEC>(xr, T, t0 + kSnakeFwdTile, tid);     // in flight while this tile is computed
    __syncthreads();
    if (4 * tid < len + 6) {
      float u[8];
      snake_up4(xs, tid, tu, u);
      snake_store4(u, a, inv_b, ve, vo, tid);
    }
    __syncthreads();
    const int pe = T - t0 + 3;                 // the first pair past the row's end
    if (t0 == 0 || pe < len + 6) {             // replicate pad of the 2x signal: v[0] on the left, v[2T-1] on the right
      if (tid < 3) {
        if (t0 == 0) ve[tid] = vo[tid] = ve[3];
        if (pe + tid < len + 6) ve[pe + tid] = vo[pe + tid] = vo[pe - 1];
      }
      __syncthreads();
    }
    if (4 * tid < len) {
      const f32x4 out = snake_down4(ve, vo, tid, td);
      float* yp = yr + t0 + 4 * tid;
      if (VEC) {                               // T % 4 == 0: len is a multiple of 4, the thread's four outputs are all inside
        *reinterpret_cast<f32x4*>(yp) = out;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (4 * tid + i < len) yp[i] = out[i];
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void aa_snake_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ alpha, const float* __restrict__ beta,
                                                          Taps12 tu, Taps12 td, int logscale, int C, int T, int nsub) {
  __shared__ __attribute__((aligned(16))) float xs[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float ve[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float vo[kSnakeFwdTile + 16];
  const int c = blockIdx.y, b = blockIdx.z;
  const int64_t row = ((int64_t)b * C + c) * T;
  aa_snake_row<VEC>(x + row, y + row, alpha, beta, tu, td, logscale, c, T, blockIdx.x * nsub * kSnakeFwdTile, nsub, xs, ve, vo);
}

// Per-item form: rows of pitch T, item b has len[b] <= T valid columns and is computed as a row of that length -- its replicate padding
// ends at len[b] - 1, tiles at or beyond len[b] do nothing (a workgroup of an empty item returns at once), and nothing at or beyond
// column len[b] is read or written.  Columns [0, len[b]) are the bits of aa_snake_kernel on the row alone with T = len[b].  The 16-byte
// path is chosen per ROW (block-uniform): the row's address depends on the pitch, the whole-vector store on len[b] % 4.
__global__ __launch_bounds__(256) void aa_snake_items_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                const float* __restrict__ alpha, const float* __restrict__ beta,
                                                                Taps12 tu, Taps12 td, int logscale, int C, int T,
                                                                const int64_t* __restrict__ len, int nsub) {
  __shared__ __attribute__((aligned(16))) float xs[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float ve[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float vo[kSnakeFwdTile + 16];
  const int c = blockIdx.y, b = blockIdx.z;
  const int n = (int)min(max(len[b], (int64_t)0), (int64_t)T);      // never past the pitch, whatever the table holds
  const int first = blockIdx.x * nsub * kSnakeFwdTile;
  if (first >= n) return;
  const int64_t row = ((int64_t)b * C + c) * T;
  const float* xr = x + row;
  float* yr = y + row;
  const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(xr) | reinterpret_cast<uintptr_t>(yr)) % 16 == 0;
  if (vec) aa_snake_row<true>(xr, yr, alpha, beta, tu, td, logscale, c, n, first, nsub, xs, ve, vo);
  else aa_snake_row<false>(xr, yr, alpha, beta, tu, td, logscale, c, n, first, nsub, xs, ve, vo);
}

// ---- three activations of ONE tensor (the heads of the three AMP blocks behind an up-sampler) ------------------------------------
// y[k] = activation(x; alpha[k], beta[k]), k = 0..2: per tile the row segment is read and the up-filter evaluated ONCE (u, eight registers),
// then each parameter set runs snake -> planes -> down-filter -> store.  4 tensors move where three launches move 6.  Each output's
// arithmetic is aa_snake_row's (the same stage bodies), so y[k] has the bits of a launch of its own.  The planes are double-buffered: set
// k writes the pair that set k - 2 read, and the barrier inside set k - 1 stands between the two, so a set costs one barrier (the pad
// patch aside) and a tile four where three separate tiles cost nine.  5 x 4 KB of LDS: eight workgroups per CU, as before.
// yvec bit k: y[k]'s rows are 16-byte aligned -- the wide store is taken per output (VEC also needs x aligned and T % 4 == 0).
struct Snake3 {
  float* y[3];
  const float* alpha[3];
  const float* beta[3];      // NULL: Snake (beta = alpha)
};

template <bool VEC>
__device__ __forceinline__ void aa_snake3_row(const float* __restrict__ xr, int64_t row, const Snake3& p, const Taps12& tu, const Taps12& td,
                                              int logscale, int c, int T, int first, int nsub, int yvec, float* xs, float* planes) {
  float a[3], inv_b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) snake_params(p.alpha[k], p.beta[k], logscale, c, a[k], inv_b[k]);
  const int tid = threadIdx.x;
  f32x4 pre = {0.f, 0.f, 0.f, 0.f};
  if (first < T) pre = snake_fetch4<VEC>(xr, T, first, tid);
  int par = 0;
  for (int sub = 0; sub < nsub; ++sub) {
    const int t0 = first + sub * kSnakeFwdTile;
    if (t0 >= T) break;
    const int len = min(kSnakeFwdTile, T - t0);
    // xs was last read before the first barrier of the previous tile's set 0: no barrier in front of this store
    *reinterpret_cast<f32x4*>(xs + 4 * tid) = pre;
    if (sub + 1 < nsub && t0 + kSnakeFwdTile < T) pre = snake_fetch4<VEC>(xr, T, t0 + kSnakeFwdTile, tid);
    __syncthreads();
    const bool pairs = 4 * tid < len + 6;
    float u[8];
    if (pairs) snake_up4(xs, tid, tu, u);
    const int pe = T - t0 + 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float* ve = planes + par * 2 * (kSnakeFwdTile + 16);
      float* vo = ve + (kSnakeFwdTile + 16);
      par ^= 1;
      if (pairs) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = u[i];
        snake_store4(v, a[k], inv_b[k], ve, vo, tid);
      }
      __syncthreads();
      if (t0 == 0 || pe < len + 6) {
        if (tid < 3) {
          if (t0 == 0) ve[tid] = vo[tid] = ve[3];
          if (pe + tid < len + 6) ve[pe + tid] = vo[pe + tid] = vo[pe - 1];
        }
        __syncthreads();
      }
      if (4 * tid < len) {
        const f32x4 out = snake_down4(ve, vo, tid, td);
        float* yp = p.y[k] + row + t0 + 4 * tid;
        if (VEC && ((yvec >> k) & 1)) {
          *reinterpret_cast<f32x4*>(yp) = out;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (4 * tid + i < len) yp[i] = out[i];
        }
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void aa_snake3_kernel(const float* __restrict__ x, Snake3 p, Taps12 tu, Taps12 td, int logscale, int C, int T,
                                                           int nsub, int yvec) {
  __shared__ __attribute__((aligned(16))) float xs[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float planes[4 * (kSnakeFwdTile + 16)];
  const int c = blockIdx.y, b = blockIdx.z;
  const int64_t row = ((int64_t)b * C + c) * T;
  aa_snake3_row<VEC>(x + row, row, p, tu, td, logscale, c, T, blockIdx.x * nsub * kSnakeFwdTile, nsub, yvec, xs, planes);
}

// per-item form, as aa_snake_items_kernel: the paths are chosen per row
__global__ __launch_bounds__(256) void aa_snake3_items_kernel(const float* __restrict__ x, Snake3 p, Taps12 tu, Taps12 td, int logscale, int C,
                                                                 int T, const int64_t* __restrict__ len, int nsub) {
  __shared__ __attribute__((aligned(16))) float xs[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float planes[4 * (kSnakeFwdTile + 16)];
  const int c = blockIdx.y, b = blockIdx.z;
  const int n = (int)min(max(len[b], (int64_t)0), (int64_t)T);
  const int first = blockIdx.x * nsub * kSnakeFwdTile;
  if (first >= n) return;
  const int64_t row = ((int64_t)b * C + c) * T;
  const float* xr = x + row;
  int yvec = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) yvec |= (int)(reinterpret_cast<uintptr_t>(p.y[k] + row) % 16 == 0) << k;
  const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(xr) % 16 == 0;
  if (vec) aa_snake3_row<true>(xr, row, p, tu, td, logscale, c, n, first, nsub, yvec, xs, planes);
  else aa_snake3_row<false>(xr, row, p, tu, td, logscale, c, n, first, nsub, 0, xs, planes);
}

// ---- activation_post + conv_post + tanh | clamp as one launch ----------------------------------------------------------------------
// y[b, t] = act(bias + sum_c sum_k w[c, k] * A[b, c, t + k - pad]), A = activation(x) inside [0, n) and conv_post's zero padding outside
// (n = T, or the item's length).  One workgroup owns W = 1008 - 2 H output columns (H = pad rounded up to 4, so W = 1000 for k = 7) of one
// item and walks the C channels in order: channel c's activation tile -- the 1008 columns from t0 = first - H, computed with
// aa_snake_row's stage bodies, the row segment of channel c + 1 in flight meanwhile -- goes to an LDS plane instead of HBM, zeroed outside
// [0, n), and every thread adds its four outputs' K taps of it: acc = fma(w[c, k], A, acc), c outer and k inner from acc = bias, which is
// conv_post_kernel's order, so y has the bits of the two launches.  The activated tensor (C x T x 4 bytes written and read again) never
// exists.  t0 is a multiple of 4 and may be negative in an item's first tile: the row segment clamps as ever, the pairs left of pair 0
// are patched with v[0] wherever pair 0 sits, and columns t < 0 are zeroed like those at or beyond n.  The weights are read through the
// scalar cache (wave-uniform addresses).
template <int KT>      // KT = 7: the vocoder's conv_post, the taps as three 16-byte LDS reads; KT = 0: any odd K with pad <= kPostMaxPad
__global__ __launch_bounds__(256) void snake_post_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ alpha,
                                                            const float* __restrict__ beta, Taps12 tu, Taps12 td, int logscale,
                                                            const float* __restrict__ w, float bias, int act, int C, int K, int T,
                                                            const int64_t* __restrict__ len) {
  __shared__ __attribute__((aligned(16))) float xs[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float ve[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float vo[kSnakeFwdTile + 16];
  __shared__ __attribute__((aligned(16))) float as[kSnakeFwdTile + 16];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int pad = (KT ? KT : K) / 2, H = (pad + 3) & ~3, W = kSnakeFwdTile - 2 * H;
  const int first = blockIdx.x * W;
  const int n = len ? (int)min(max(len[b], (int64_t)0), (int64_t)T) : T;
  float* yb = y + (int64_t)b * T;
  if (first >= n) {                            // a tile wholly behind the item's end (block-uniform): zeros
    for (int t = first + tid; t < min(first + W, T); t += 256) yb[t] = 0.f;
    return;
  }
  const int t0 = first - H;
  const int alen = min(kSnakeFwdTile, n - t0);       // activation columns t0 .. t0 + alen - 1 (those below 0 are computed and zeroed)
  const float* xr = x + (int64_t)b * C * T;
  const bool vec = T % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;      // every row then starts on a 16-byte boundary
  float acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = bias;
  f32x4 pre = vec ? snake_fetch4<true>(xr, n, t0, tid) : snake_fetch4<false>(xr, n, t0, tid);
  const int pz = 3 - t0;                       // the pair of sample 0, when the tile holds it
  const int pe = n - t0 + 3;                   // the first pair past the row's end
  for (int c = 0; c < C; ++c) {
    float a, inv_b;
    snake_params(alpha, beta, logscale, c, a, inv_b);
    // xs / ve+vo / as were last read two / one / three barriers ago
    *reinterpret_cast<f32x4*>(xs + 4 * tid) = pre;
    if (c + 1 < C) {
      xr += T;
      pre = vec ? snake_fetch4<true>(xr, n, t0, tid) : snake_fetch4<false>(xr, n, t0, tid);
    }
    __syncthreads();
    if (4 * tid < alen + 6) {
      float u[8];
      snake_up4(xs, tid, tu, u);
      snake_store4(u, a, inv_b, ve, vo, tid);
    }
    __syncthreads();
    if (t0 <= 0 || pe < alen + 6) {
      if (tid < 3) {
        if (t0 <= 0) ve[pz - 1 - tid] = vo[pz - 1 - tid] = ve[pz];
        if (pe + tid < alen + 6) ve[pe + tid] = vo[pe + tid] = vo[pe - 1];
      }
      __syncthreads();
    }
    if (4 * tid < kSnakeFwdTile) {
      f32x4 out = {0.f, 0.f, 0.f, 0.f};
      if (4 * tid < alen) out = snake_down4(ve, vo, tid, td);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * tid + i;
        if (t < 0 || t >= n) out[i] = 0.f;
      }
      *reinterpret_cast<f32x4*>(as + 4 * tid) = out;
    }
    __syncthreads();
    if (4 * tid < W) {
      const float* wc = w + c * (KT ? KT : K);
      if (KT == 7) {                           // H = 4, pad = 3: output 4 tid + e reads as[4 tid + e + 1 + k]
        float v[12];
        lds_read3_b128(as + 4 * tid, v);
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          const float wv = wc[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv, v[e + 1 + k], acc[e]);
        }
      } else {
        const float* ap = as + 4 * tid + (H - pad);
        for (int k = 0; k < K; ++k) {
          const float wv = wc[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv, ap[e + k], acc[e]);
        }
      }
    }
  }
  if (4 * tid < W) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = first + 4 * tid + e;
      if (t < T) {
        const float v = act == 2 ? tanhf(acc[e]) : (act == 3 ? fminf(fmaxf(acc[e], -1.f), 1.f) : acc[e]);
        yb[t] = t < n ? v : 0.f;
      }
    }
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
  // three tiles per workgroup (the next one's row segment is in flight while one is computed).  On the MI355X, us per launch at batch 32
  // for nsub = 2 / 3 / 4: 128 x 5888: 45.1 / 45.3 / 55.9 (four leave the second workgroup of a row 1.84 tiles against 4), 64 x 11776:
  // 44.1 / 42.6 / 42.1, 32 x 23552: 43.2 / 42.1 / 41.2 (profiles/aa_snake_blocked.txt)
  constexpr int nsub = 3;
  constexpr int span = kSnakeFwdTile * nsub;
  dim3 grid((unsigned)((T + span - 1) / span), (unsigned)C, (unsigned)B);
  // 16-byte global accesses need every row to start on a 16-byte boundary; the other instantiation computes the same bits
  const bool vec = T % 4 == 0 && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
  {
    ProfScope ps("aa_snake", s, 0.0, 8.0 * (double)B * C * (double)T);
    if (vec) hipLaunchKernelGGL(aa_snake_kernel<true>, grid, dim3(256), 0, s, x, y, alpha, beta, tu, td, logscale, C, (int)T, nsub);
    else hipLaunchKernelGGL(aa_snake_kernel<false>, grid, dim3(256), 0, s, x, y, alpha, beta, tu, td, logscale, C, (int)T, nsub);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// x, y (B, C, T) with T the row pitch; len: B device int64, item b's valid columns (clamped into [0, T] by the kernel)
int launch_aa_snake_items(const float* x, float* y, const float* alpha, const float* beta, const float* up_taps_host,
                          const float* down_taps_host, int logscale, int B, int C, int64_t T, const int64_t* len, hipStream_t s) {
  DMEL_CHECK_ARG(x && y && alpha && up_taps_host && down_taps_host && len, "aa_snake_items: NULL argument");
  DMEL_CHECK_ARG(B > 0 && C > 0 && T > 0 && B <= 65535 && C <= 65535 && T < ((int64_t)1 << 30), "aa_snake_items: bad shape");
  Taps12 tu, td;
  for (int i = 0; i < 12; ++i) { tu.f[i] = 2.f * up_taps_host[i]; td.f[i] = down_taps_host[i]; }
  constexpr int nsub = 3;      // as launch_aa_snake
  constexpr int span = kSnakeFwdTile * nsub;
  dim3 grid((unsigned)((T + span - 1) / span), (unsigned)C, (unsigned)B);      // sized by the pitch: the lengths stay on the device
  {
    ProfScope ps("aa_snake", s, 0.0, 8.0 * (double)B * C * (double)T);
    hipLaunchKernelGGL(aa_snake_items_kernel, grid, dim3(256), 0, s, x, y, alpha, beta, tu, td, logscale, C, (int)T, len, nsub);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// y[k] (B, C, T) = activation(x; alpha[k], beta[k]) for three parameter sets in one launch; len (nullable) as launch_aa_snake_items.
// The outputs must not overlap x or one another.
int launch_aa_snake3(const float* x, float* const y[3], const float* const alpha[3], const float* const beta[3], const float* up_taps_host,
                     const float* down_taps_host, int logscale, int B, int C, int64_t T, const int64_t* len, hipStream_t s) {
  DMEL_CHECK_ARG(x && y && alpha && beta && up_taps_host && down_taps_host, "aa_snake3: NULL argument");
  DMEL_CHECK_ARG(y[0] && y[1] && y[2] && alpha[0] && alpha[1] && alpha[2], "aa_snake3: NULL output or alpha");
  DMEL_CHECK_ARG(y[0] != y[1] && y[0] != y[2] && y[1] != y[2] && x != y[0] && x != y[1] && x != y[2], "aa_snake3: x and the outputs must be distinct");
  DMEL_CHECK_ARG(B > 0 && C > 0 && T > 0 && B <= 65535 && C <= 65535 && T < ((int64_t)1 << 30), "aa_snake3: bad shape");
  Taps12 tu, td;
  for (int i = 0; i < 12; ++i) { tu.f[i] = 2.f * up_taps_host[i]; td.f[i] = down_taps_host[i]; }
  Snake3 p;
  int yvec = 0;
  for (int k = 0; k < 3; ++k) {
    p.y[k] = y[k]; p.alpha[k] = alpha[k]; p.beta[k] = beta[k];
    yvec |= (int)(reinterpret_cast<uintptr_t>(y[k]) % 16 == 0) << k;
  }
  constexpr int nsub = 3;      // as launch_aa_snake
  constexpr int span = kSnakeFwdTile * nsub;
  dim3 grid((unsigned)((T + span - 1) / span), (unsigned)C, (unsigned)B);
  const bool vec = T % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
  {
    ProfScope ps("aa_snake", s, 0.0, 16.0 * (double)B * C * (double)T);      // one read, three writes
    if (len) hipLaunchKernelGGL(aa_snake3_items_kernel, grid, dim3(256), 0, s, x, p, tu, td, logscale, C, (int)T, len, nsub);
    else if (vec) hipLaunchKernelGGL(aa_snake3_kernel<true>, grid, dim3(256), 0, s, x, p, tu, td, logscale, C, (int)T, nsub, yvec);
    else hipLaunchKernelGGL(aa_snake3_kernel<false>, grid, dim3(256), 0, s, x, p, tu, td, logscale, C, (int)T, nsub, 0);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

// y (B, 1, T) = act(conv_post(activation(x))), x (B, C, T); len (nullable) as launch_conv_post: y[b, len[b]:] = 0.  Accepts what
// launch_conv_post accepts up to K = 2 * kPostMaxPad + 1 taps.
constexpr int kPostMaxPad = 128;
int launch_snake_post(const float* x, float* y, const float* alpha, const float* beta, const float* up_taps_host, const float* down_taps_host,
                      int logscale, const float* w_dev, float bias, int act, int B, int C, int K, int64_t T, const int64_t* len, hipStream_t s) {
  DMEL_CHECK_ARG(x && y && alpha && up_taps_host && down_taps_host && w_dev, "snake_post: NULL argument");
  DMEL_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && K > 0 && (K % 2) == 1 && T > 0 && T < ((int64_t)1 << 30), "snake_post: bad shape");
  DMEL_CHECK_ARG((size_t)C * K * sizeof(float) <= 48 * 1024, "snake_post: weight table too large");
  DMEL_CHECK_ARG(K / 2 <= kPostMaxPad, "snake_post: more than %d taps", 2 * kPostMaxPad + 1);
  Taps12 tu, td;
  for (int i = 0; i < 12; ++i) { tu.f[i] = 2.f * up_taps_host[i]; td.f[i] = down_taps_host[i]; }
  const int W = kSnakeFwdTile - 2 * ((K / 2 + 3) & ~3);
  dim3 grid((unsigned)((T + W - 1) / W), (unsigned)B);
  {
    ProfScope ps("small", s, 0.0, 4.0 * B * (double)T * (C + 1));
    if (K == 7) hipLaunchKernelGGL(snake_post_kernel<7>, grid, dim3(256), 0, s, x, y, alpha, beta, tu, td, logscale, w_dev, bias, act, C, K, (int)T, len);
    else hipLaunchKernelGGL(snake_post_kernel<0>, grid, dim3(256), 0, s, x, y, alpha, beta, tu, td, logscale, w_dev, bias, act, C, K, (int)T, len);
  }
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}

}  // namespace dmel

extern "C" int dmel_aa_snake3_forward(const float* x, float* y0, float* y1, float* y2, const float* alpha0, const float* beta0,
                                      const float* alpha1, const float* beta1, const float* alpha2, const float* beta2,
                                      const float* up_filter12_host, const float* down_filter12_host, int logscale, int B, int C, int64_t T,
                                      void* stream) {
  float* const y[3] = {y0, y1, y2};
  const float* const al[3] = {alpha0, alpha1, alpha2};
  const float* const be[3] = {beta0, beta1, beta2};
  return dmel::launch_aa_snake3(x, y, al, be, up_filter12_host, down_filter12_host, logscale, B, C, T, nullptr, (hipStream_t)stream);
}

extern "C" int dmel_aa_snake3_forward_items(const float* x, float* y0, float* y1, float* y2, const float* alpha0, const float* beta0,
                                            const float* alpha1, const float* beta1, const float* alpha2, const float* beta2,
                                            const float* up_filter12_host, const float* down_filter12_host, int logscale, int B, int C,
                                            int64_t T, const int64_t* lengths_dev, void* stream) {
  DMEL_CHECK_ARG(lengths_dev, "aa_snake3_forward_items: NULL lengths");
  float* const y[3] = {y0, y1, y2};
  const float* const al[3] = {alpha0, alpha1, alpha2};
  const float* const be[3] = {beta0, beta1, beta2};
  return dmel::launch_aa_snake3(x, y, al, be, up_filter12_host, down_filter12_host, logscale, B, C, T, lengths_dev, (hipStream_t)stream);
}

static int snake_post_entry(const float* x, const float* alpha, const float* beta, const float* up, const float* down, int logscale,
                            const float* w_dev, float bias, int act, float* y, int B, int C, int K, int64_t T, const int64_t* len, void* stream) {
  DMEL_CHECK_ARG(act == 0 || act == 2 || act == 3, "snake_post: act must be 0 (none), 2 (tanh) or 3 (clamp to [-1, 1])");
  return dmel::launch_snake_post(x, y, alpha, beta, up, down, logscale, w_dev, bias, act, B, C, K, T, len, (hipStream_t)stream);
}

extern "C" int dmel_snake_post_forward(const float* x, const float* alpha, const float* beta, const float* up_filter12_host,
                                       const float* down_filter12_host, int logscale, const float* w_dev, float bias, int act, float* y, int B,
                                       int C, int K, int64_t T, void* stream) {
  return snake_post_entry(x, alpha, beta, up_filter12_host, down_filter12_host, logscale, w_dev, bias, act, y, B, C, K, T, nullptr, stream);
}

extern "C" int dmel_snake_post_forward_items(const float* x, const float* alpha, const float* beta, const float* up_filter12_host,
                                             const float* down_filter12_host, int logscale, const float* w_dev, float bias, int act, float* y,
                                             int B, int C, int K, int64_t T, const int64_t* lengths_dev, void* stream) {
  DMEL_CHECK_ARG(lengths_dev, "snake_post_forward_items: NULL lengths");
  return snake_post_entry(x, alpha, beta, up_filter12_host, down_filter12_host, logscale, w_dev, bias, act, y, B, C, K, T, lengths_dev, stream);
}

extern "C" int dmel_aa_snake_items_f32(const float* x, float* y, const float* alpha, const float* beta, const float* up_filter12_host,
                                       const float* down_filter12_host, int logscale, int B, int C, int64_t T, const int64_t* lengths_dev,
                                       void* stream) {
  return dmel::launch_aa_snake_items(x, y, alpha, beta, up_filter12_host, down_filter12_host, logscale, B, C, T, lengths_dev,
                                     (hipStream_t)stream);
}

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
