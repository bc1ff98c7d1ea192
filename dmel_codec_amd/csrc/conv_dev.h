// Device-side pieces shared by the convolution kernels (conv_igemm.hip, conv_snake.hip): kernel arguments, the epilogue, the
// workgroup -> tile map.  Internal to the library.
#pragma once
#include "conv.h"

#include <cstdlib>
#include <type_traits>

namespace dmel {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct SegArgs {
  const float* x;
  int64_t bstride, cstride, Tin;
  const int64_t* in_len;
  float in_scale;
  int Cin, nchunk, taps, dil, pad_left, tstride, toff;
  const uint32_t* in_absmax;    // fp16 split over a gradient tensor (segment 0 only): see conv.h SegRun
  // Pre-split input (conv.h SegRun::xp): the operand already as two fp16 planes in B-fragment order, [piece][b][channel / 8][t] x 16 bytes
  const uint4* xp;
  int64_t xp_plane;             // uint4 between the two pieces
  int xp_g8;                    // 8-channel groups per batch item
};

struct KArgs {
  SegArgs seg[2];
  int nseg, steps, mtiles;
  int gx, gy, gz, xcd_chunk;   // logical grid (column tiles, m blocks, batch); xcd_chunk > 0: 1-D XCD-chunked launch
  const float* w;
  const void* w16;
  const void* w48;
  const void* w32h;
  const float* bias;
  int64_t Tcols;
  int mode, act, C, RP, phases, out_tstride, phase_base, accumulate, len_div, skip_first;
  float out_div;
  float* y;
  int64_t y_bs, y_cs, Tout;
  const float* res;
  int64_t res_bs, res_cs;
  const float* row_scale;
  const int64_t* out_len;
  float* skip;
  int fold_pitch, fold_valid;
  // paired modes: also (yp_only: instead) write the output as pre-split fp16 planes for the convolution that reads it next
  uint4* yp;
  int64_t yp_plane;
  int yp_g8, yp_only;
  // per-item column windows (conv.h ConvRun::win), read by conv_bf16_kernel<WIN> only: row b / len_div of `win`, win_stride int32 each
  const int32_t* win;
  int win_stride, win_shift, win_end, win_valid[2];
  int fast;                    // conv_fastpath_enabled() at launch: full tiles / interior chunks of the fp16-split kernels skip the edge code
  int row_u;                   // PackDesc::row_u: > 1 = phase-minor rows of a stride-row_u transposed convolution (epi_phase_rows)
};

__device__ __forceinline__ float act_apply(float v, int act) {
  switch (act) {
    case ACT_SILU: return v / (1.f + expf(-v));
    case ACT_TANH: return tanhf(v);
    case ACT_CLAMP1: return fminf(fmaxf(v, -1.f), 1.f);
    case ACT_GELU: return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    default: return v;
  }
}

// folded batch (ConvRun::fold_pitch): is output column q one of the zero columns between two items?
__device__ __forceinline__ bool in_gap(const KArgs& a, int q) {
  return a.fold_pitch > 0 && (q % a.fold_pitch) >= a.fold_valid;
}

// DMEL_CONV_FASTPATH=0: every tile and every staged chunk of the fp16-split kernels takes the edge code (clamps, masks and selects per
// element), as a tile that straddles the end of a row does anyway; unset or any other value: tiles / chunks that lie wholly inside the
// tensor take the forms without them (epi_full_tile below, the interior staging of conv_bf16_kernel / conv_pc_kernel).  Same expressions
// in the same order on both: bit-identical (tests/test_gpu_conv_fastpath.py).  Read per call.
inline bool conv_fastpath_enabled() {
  const char* e = getenv("DMEL_CONV_FASTPATH");
  return !(e && e[0] == '0' && e[1] == 0);
}

// Lean LINEAR epilogue of one 32 x (32 NT) tile that lies WHOLLY inside the output: its 32 rows below C, its columns below Tcols, Tout
// and out_len, no fold gap.  Nothing is clamped, masked or selected, and the flags that are uniform over the launch (residual, running
// sum, 1 / out_div) are template arguments: a launch with out_div == 1 executes no division (v / 1.f == v exactly, so skipping it
// keeps the bits; the vocoder divides in the last convolution of a stage only).  Addresses are a wave-uniform row base (scalar registers:
// mtile, the row's constant offset and the channel stride are uniform) plus ONE 32-bit lane byte offset per tensor, computed once from 4 h and
// the lane's column: no per-row vector multiply, sign extension or 64-bit vector add.  Value expressions and their order are those of the
// edge loop in conv_epilogue.  As there, all residual / running-sum loads of RB rows are issued before the first use.
// The 32-bit lane offset of a load / store whose base is wave-uniform, as a value the compiler cannot look through (no instruction is
// emitted).  Seen through, (uniform base) + (lane offset) is re-associated into a 64-bit lane pointer that is hoisted, and every row /
// every load then pays a 64-bit vector add for its uniform part; opaque, the access takes the uniform base as its scalar address
// operand and the offset as its 32-bit vector one (global_load_dword v, v_off, s[base:base+1]).
__device__ __forceinline__ uint32_t lane_off(uint32_t off) {
  asm volatile("" : "+v"(off));
  return off;
}

template <int NT, int RB, bool RES, bool ACC, bool DIV>
__device__ __forceinline__ void epi_full_tile(const KArgs& a, const floatx16 (&acc)[NT], int mtile, float* yb, const float* rb, uint32_t yoff,
                                              uint32_t roff, uint32_t boff) {
  const int ycs = (int)a.y_cs, rcs = (int)a.res_cs;      // int products: one item's offsets stay below 2^31 (launch_conv checks)
  const float* bias_t = a.bias + mtile;
  float* yt = yb + mtile * ycs;
  const float* rt = RES ? rb + mtile * rcs : nullptr;
#pragma unroll
  for (int g = 0; g < 16 / RB; ++g) {
    float bias[RB], rv[RB][NT], ov[RB][NT];
#pragma unroll
    for (int k = 0; k < RB; ++k) {
      const int r = g * RB + k, row = (r & 3) + 8 * (r >> 2);       // accumulator register r -> row `row` + 4 h of the tile
      bias[k] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(bias_t + row) + lane_off(boff));
      if constexpr (RES) {
        const float* rr = rt + row * rcs;
        const uint32_t ro = lane_off(roff);
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) rv[k][ni] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rr + ni * 32) + ro);
      }
      if constexpr (ACC) {
        const float* yr = yt + row * ycs;
        const uint32_t yo = lane_off(yoff);
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) ov[k][ni] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(yr + ni * 32) + yo);
      }
    }
#pragma unroll
    for (int k = 0; k < RB; ++k) {
      const int r = g * RB + k, row = (r & 3) + 8 * (r >> 2);
      float* yr = yt + row * ycs;
      const uint32_t yo = lane_off(yoff);
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        float v = acc[ni][r] + bias[k];
        if constexpr (RES) v += rv[k][ni];
        if constexpr (ACC) v += ov[k][ni];
        if constexpr (DIV) v = v / a.out_div;
        *reinterpret_cast<float*>(reinterpret_cast<char*>(yr + ni * 32) + yo) = v;
      }
    }
  }
}

// Phase-minor rows (PackDesc::row_u = U: packed row m = co U + ph is sample q U + ph of channel co): one 32 x (32 NT) tile that lies WHOLLY
// inside the output, in the manner of epi_full_tile.  With rows (r & 3) + 8 (r >> 2) + 4 h in accumulator register r, a lane holds V = min(U, 4)
// consecutive samples of one channel in V consecutive registers:
//   U = 8: registers 4 g .. 4 g + 3 are phases 4 h .. 4 h + 3 of channel g of the tile's four    -> one 16-byte store; the two half-waves
//          interleave, so a wave store is 1 KiB contiguous
//   U = 4: registers 4 g .. 4 g + 3 are phases 0 .. 3 of channel 2 g + h of the tile's eight    -> one 16-byte store, 512 B per channel
//   U = 2: registers 2 g, 2 g + 1 are phases 0, 1 of channel (g & 1) + 4 (g >> 1) + 2 h of sixteen -> one 8-byte store, 256 B per channel
// The channel's row base is wave-uniform (scalar), the lane offset (its h part of the channel, its column, its first phase) one 32-bit
// value computed once by the caller; the bias is read once per channel; no division, no flag.  The value is acc + bias, as in the edge loop.
template <int U, int NT>
__device__ __forceinline__ void epi_phase_tile(const KArgs& a, const floatx16 (&acc)[NT], int mtile, float* yb, uint32_t yoff, uint32_t boff) {
  constexpr int V = U >= 4 ? 4 : 2;
  typedef float vecf __attribute__((ext_vector_type(V)));
  const int ycs = (int)a.y_cs;
  const float* bias_t = a.bias + mtile;
  float* yt = yb + (mtile / U) * ycs;
#pragma unroll
  for (int g = 0; g < 16 / V; ++g) {
    const int r0 = g * V, row0 = (r0 & 3) + 8 * (r0 >> 2);        // first register of the group -> row `row0` + 4 h of the tile
    const float bias = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(bias_t + row0) + lane_off(boff));
    float* yr = yt + (row0 / U) * ycs;
    const uint32_t yo = lane_off(yoff);
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      vecf v;
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = acc[ni][r0 + j] + bias;
      *reinterpret_cast<vecf*>(reinterpret_cast<char*>(yr + ni * 32 * U) + yo) = v;
    }
  }
}

// The LINEAR epilogue of a launch with phase-minor rows: full tiles of an output whose base, batch stride and row pitch are aligned to the
// vector store take epi_phase_tile; a row-edge or column-edge tile, an unaligned output, a launch with DMEL_CONV_FASTPATH=0 take one store per
// element with the same value expression.  (launch_conv refuses every epilogue option but out_len / fold with row_u > 1.)
template <int MT, int NT>
__device__ __forceinline__ void epi_phase_rows(const KArgs& a, const floatx16 (&acc)[MT][NT], int mrow0, int colbase, int b, int olim, int h) {
  const int u = a.row_u, sh = u == 8 ? 3 : u == 4 ? 2 : 1;
  const int tcols = (int)a.Tcols, tout = (int)a.Tout, ycs = (int)a.y_cs;
  const int bu = __builtin_amdgcn_readfirstlane(b);
  float* ybu = a.y + (int64_t)bu * a.y_bs;
  const int col0 = __builtin_amdgcn_readfirstlane(colbase - (int)(__lane_id() & 31));
  const uint32_t vbytes = u >= 4 ? 16u : 8u;
  const bool aligned = (((uint32_t)reinterpret_cast<uintptr_t>(a.y) | (uint32_t)(a.y_bs * 4) | (uint32_t)(a.y_cs * 4)) & (vbytes - 1)) == 0;
  const bool full_cols = a.fast && aligned && a.fold_pitch == 0 && col0 + NT * 32 <= tcols && (int64_t)(col0 + NT * 32) * u <= min(tout, olim) &&
                         tout <= (1 << 28) && a.y_cs < (1 << 27);      // the lane's BYTE offset (two rows + a sample) fits 32 bits
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) {
    const int mtile = mrow0 + mi * 32;
    if (mtile >= a.mtiles * 32) continue;
    const int mt = __builtin_amdgcn_readfirstlane(mtile);
    if (full_cols && mt + 32 <= a.C) {
      const uint32_t boff = (uint32_t)(16 * h);      // bytes
      if (u == 8) epi_phase_tile<8, NT>(a, acc[mi], mt, ybu, (uint32_t)(colbase * 8 + 4 * h) * 4u, boff);
      else if (u == 4) epi_phase_tile<4, NT>(a, acc[mi], mt, ybu, (uint32_t)(h * ycs + colbase * 4) * 4u, boff);
      else epi_phase_tile<2, NT>(a, acc[mi], mt, ybu, (uint32_t)(2 * h * ycs + colbase * 2) * 4u, boff);
      continue;
    }
    float* yb = a.y + (int64_t)b * a.y_bs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mtile + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (m >= a.C) continue;
      const int co = m >> sh, ph = m & (u - 1);
      const float bias = a.bias[m];
      float* yrow = yb + (int64_t)co * ycs;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int q = colbase + ni * 32;
        const int64_t t = (int64_t)q * u + ph;
        if (q >= tcols || t >= tout) continue;
        float v = acc[mi][ni][r] + bias;
        if (t >= olim || in_gap(a, q)) v = 0.f;
        yrow[t] = v;
      }
    }
  }
}

// ------------------------------------------------------------------ epilogue (shared by both kernels)
// Lane (h, l31) holds, for each 32x32 tile, column l31 and rows (r&3) + 8*(r>>2) + 4*h, r = 0..15.
// Row-only quantities (bias, row offsets, channel map) are computed once per row, outside the column loop.
// LEAN_ONLY: the caller guarantees the lean LINEAR case (no activation, row scale, phases or output stride): the general loop is not compiled
// FAST: compile epi_full_tile for the lean LINEAR tiles that lie wholly inside the output (the fp16-split kernels; taken when a.fast is set)
template <int MT, int NT, int MODE, int RB = 4, bool LEAN_ONLY = false, bool FAST = false>      // RB: rows whose residual / running-sum loads are in flight together (lean LINEAR path)
__device__ __forceinline__ void conv_epilogue(const KArgs& a, floatx16 (&acc)[MT][NT], int mrow0, int colbase, int b, int lb,
                                              int h) {
  const int tcols = (int)a.Tcols;
  if (MODE == EPI_LINEAR) {
    const int olim = a.out_len ? (int)min(a.out_len[lb], (int64_t)0x7fffffff) : 0x7fffffff;
    float* yb = a.y + (int64_t)b * a.y_bs;
    const float* rb = a.res ? a.res + (int64_t)b * a.res_bs : nullptr;
    const int ycs = (int)a.y_cs, rcs = (int)a.res_cs, tout = (int)a.Tout;
    if constexpr (!LEAN_ONLY) {
      if (a.row_u > 1) {        // phase-minor rows: a transposed convolution in one image
        epi_phase_rows<MT, NT>(a, acc, mrow0, colbase, b, olim, h);
        return;
      }
    }
    // The common case (plain conv, optionally + residual: 5 of 6 vocoder convs, every WaveNet projection) gets a loop
    // with no per-element flag tests: the general loop below spends more time in uniform branches than in stores.
    const bool lean = LEAN_ONLY || (a.act == ACT_NONE && !a.row_scale && a.phases == 1 && a.out_tstride == 1 && a.phase_base == 0);
    if (lean) {
      const int tlim = min(tcols, tout);
      bool colok[NT], live[NT];
      int cq[NT];               // column offsets clamped into the row, so residual loads need no predicate
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        colok[ni] = colbase + ni * 32 < tlim;
        live[ni] = colbase + ni * 32 < olim && !in_gap(a, colbase + ni * 32);
        cq[ni] = min(colbase + ni * 32, tlim - 1);
      }
      // full-tile test, wave-uniform: the wave's first column (the lane's column less its index in the half-wave) and its row tile
      bool full_cols = false;
      float* ybu = nullptr;            // the item's bases from a batch index in a scalar register: with the XCD-chunked grid b is the result of
      const float* rbu = nullptr;      // vector divisions, and a base in vector registers cannot be the scalar address operand of a load / store
      if constexpr (FAST) {
        const int bu = __builtin_amdgcn_readfirstlane(b);
        ybu = a.y + (int64_t)bu * a.y_bs;
        rbu = a.res ? a.res + (int64_t)bu * a.res_bs : nullptr;
        const int col0 = __builtin_amdgcn_readfirstlane(colbase - (int)(__lane_id() & 31));
        full_cols = a.fast && a.fold_pitch == 0 && col0 + NT * 32 <= min(tlim, olim) &&
                    tlim <= (1 << 28) && a.y_cs < (1 << 27) && a.res_cs < (1 << 27);      // the lane's BYTE offsets (4 rows + a column) fit 32 bits
      }
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) {
        const int mtile = mrow0 + mi * 32;
        if (mtile >= a.mtiles * 32) continue;
        if constexpr (FAST) {
          const int mt = __builtin_amdgcn_readfirstlane(mtile);
          if (full_cols && mt + 32 <= a.C) {
            const uint32_t yoff = (uint32_t)(4 * h * ycs + colbase) * 4u, roff = (uint32_t)(4 * h * rcs + colbase) * 4u, boff = (uint32_t)(16 * h);      // bytes
            auto tile = [&](auto R, auto A, auto D) {
              epi_full_tile<NT, RB, decltype(R)::value, decltype(A)::value, decltype(D)::value>(a, acc[mi], mt, ybu, rbu, yoff, roff, boff);
            };
            constexpr std::true_type T{};
            constexpr std::false_type F{};
            switch ((rb ? 4 : 0) | (a.accumulate ? 2 : 0) | (a.out_div != 1.f ? 1 : 0)) {
              case 0: tile(F, F, F); break;
              case 1: tile(F, F, T); break;
              case 2: tile(F, T, F); break;
              case 3: tile(F, T, T); break;
              case 4: tile(T, F, F); break;
              case 5: tile(T, F, T); break;
              case 6: tile(T, T, F); break;
              default: tile(T, T, T); break;
            }
            continue;
          }
        }
        // RB rows at a time: all their residual / running-sum loads are issued before the first use, so the wave meets the HBM latency
        // 16 / RB times per tile.  The fp16-split kernel asks for 8 (its second accumulator set is dead here: -0.15 ms per bench step); for the
        // others 8 rows cost 32 registers and a wave of occupancy (100 -> 132 VGPRs on the 128 x 96 tile), so they keep 4.
#pragma unroll
        for (int g = 0; g < 16 / RB; ++g) {
          float bias[RB], rv[RB][NT];
          int co[RB];
          float ov[RB][NT];          // previous output, for the running sum of the AMP branches (accumulate)
#pragma unroll
          for (int k = 0; k < RB; ++k) {
            const int r = g * RB + k;                                  // accumulator register -> row (r & 3) + 8 (r >> 2) + 4 h
            co[k] = mtile + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int cc = min(co[k], a.C - 1);
            bias[k] = a.bias[cc];
            if (rb) {
#pragma unroll
              for (int ni = 0; ni < NT; ++ni) rv[k][ni] = rb[cc * rcs + cq[ni]];
            }
            if (a.accumulate) {
#pragma unroll
              for (int ni = 0; ni < NT; ++ni) ov[k][ni] = yb[cc * ycs + cq[ni]];
            }
          }
#pragma unroll
          for (int k = 0; k < RB; ++k) {
            if (co[k] >= a.C) continue;
            float* yrow = yb + co[k] * ycs + colbase;
#pragma unroll
            for (int ni = 0; ni < NT; ++ni) {
              float v = acc[mi][ni][g * RB + k] + bias[k];
              if (rb) v += rv[k][ni];
              if (a.accumulate) v += ov[k][ni];
              if (a.out_div != 1.f) v = v / a.out_div;
              if (colok[ni]) yrow[ni * 32] = live[ni] ? v : 0.f;
            }
          }
        }
      }
      return;
    }
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      const int mtile = mrow0 + mi * 32;
      if (mtile >= a.mtiles * 32) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mtile + (r & 3) + 8 * (r >> 2) + 4 * h;
        int ph = 0, co = m;
        if (a.phases > 1) { ph = m / a.RP; co = m - ph * a.RP; }
        if (co >= a.C || ph >= a.phases) continue;
        const float bias = a.bias[m];
        const float rs = a.row_scale ? a.row_scale[co] : 1.f;
        const int tph = a.phase_base + ph;
        float* yrow = yb + co * ycs;
        const float* rrow = rb ? rb + co * rcs : nullptr;
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const int q = colbase + ni * 32;
          const int t = q * a.out_tstride + tph;
          if (q >= tcols || t >= tout) continue;
          float v = act_apply(acc[mi][ni][r] + bias, a.act) * rs;
          if (rrow) v += rrow[t];
          if (a.accumulate) v += yrow[t];
          if (a.out_div != 1.f) v = v / a.out_div;
          if (t >= olim || in_gap(a, q)) v = 0.f;
          yrow[t] = v;
        }
      }
    }
  } else {
    float* yb = a.y + (int64_t)b * a.y_bs;
    float* sb = (MODE == EPI_RESSKIP) ? a.skip + (int64_t)b * a.y_bs : nullptr;
    const int ycs = (int)a.y_cs;
    bool gap[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) gap[ni] = in_gap(a, colbase + ni * 32);
    typedef _Float16 ep_f16x2 __attribute__((ext_vector_type(2)));
    typedef float ep_f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      const int mtile = mrow0 + mi * 32;
      if (mtile >= a.mtiles * 32) continue;
      const int q32 = mtile >> 5;
      // A lane holds, of each 8-channel group of the tile, FOUR consecutive channels (4 h .. 4 h + 3: accumulator registers r0 .. r0 + 3,
      // partner rows in r0 + 4 .. r0 + 7), i.e. one 8-byte half of the group's 16-byte unit in the pre-split plane layout.
#pragma unroll
      for (int gs = 0; gs < 2; ++gs) {
        const int r0 = gs * 8;
        const int c0 = q32 * 16 + gs * 8 + 4 * h;
        if (c0 >= a.C) continue;
        float b0[4], b1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int rho = j + 8 * (r0 >> 2) + 4 * h;
          b0[j] = a.bias[mtile + rho];
          b1[j] = a.bias[mtile + rho + 8];
        }
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          const int q = colbase + ni * 32;
          if (q >= tcols) continue;
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = 0.f;
            if (c0 + j >= a.C) continue;
            const float v0 = acc[mi][ni][r0 + j] + b0[j];
            const float v1 = acc[mi][ni][r0 + j + 4] + b1[j];
            float* yrow = yb + (c0 + j) * ycs;
            if (MODE == EPI_GATE) {
              o[j] = gap[ni] ? 0.f : (1.f / (1.f + expf(-v0))) * tanhf(v1);
              if (!a.yp_only) yrow[q] = o[j];
            } else {
              float* srow = sb + (c0 + j) * ycs;
              o[j] = gap[ni] ? 0.f : (yrow[q] + v0) / 1.41421356237309504880f;
              yrow[q] = o[j];
              srow[q] = gap[ni] ? 0.f : (a.skip_first ? v1 : srow[q] + v1);
            }
          }
          if (a.yp) {
            // the operand split of conv_bf16_kernel<NP = 2>::store_x, done once here instead of once per row block of the reader
#pragma clang fp contract(off)
            const float s0 = o[0] * kF16XScale, s1 = o[1] * kF16XScale, s2 = o[2] * kF16XScale, s3 = o[3] * kF16XScale;
            const ep_f16x2 h01 = __builtin_convertvector((ep_f32x2){s0, s1}, ep_f16x2), h23 = __builtin_convertvector((ep_f32x2){s2, s3}, ep_f16x2);
            const ep_f16x2 l01 = __builtin_convertvector((ep_f32x2){(s0 - (float)h01[0]) * kF16LoScale, (s1 - (float)h01[1]) * kF16LoScale}, ep_f16x2);
            const ep_f16x2 l23 = __builtin_convertvector((ep_f32x2){(s2 - (float)h23[0]) * kF16LoScale, (s3 - (float)h23[1]) * kF16LoScale}, ep_f16x2);
            uint2* dst = reinterpret_cast<uint2*>(a.yp + ((int64_t)b * a.yp_g8 + (c0 >> 3)) * tcols + q) + h;
            *dst = make_uint2(__builtin_bit_cast(uint32_t, h01), __builtin_bit_cast(uint32_t, h23));
            *(dst + 2 * a.yp_plane) = make_uint2(__builtin_bit_cast(uint32_t, l01), __builtin_bit_cast(uint32_t, l23));
          }
        }
      }
    }
  }
}

// Workgroup -> (column tile, m block, batch item).  Plain 3-D launch, or (xcd_chunk > 0) a 1-D launch in which the
// hardware's round-robin of consecutive workgroup ids over the 8 XCDs is undone: the m-block-major work list is cut
// into 8 contiguous chunks and XCD label j = id % 8 walks chunk j, so one XCD's L2 holds a contiguous 1/8 of the
// weight rows (and re-reads each x tile for its few m blocks) instead of every XCD streaming all weights through the
// Infinity Cache.  Purely a locality choice: any placement gives the same result.
__device__ __forceinline__ bool conv_block_coords(const KArgs& a, int& tile_n, int& mblk, int& b) {
  if (a.xcd_chunk <= 0) {
    tile_n = blockIdx.x; mblk = blockIdx.y; b = blockIdx.z;
    return true;
  }
  const int id = blockIdx.x;
  const int w = (id & 7) * a.xcd_chunk + (id >> 3);
  const int per_m = a.gx * a.gz;
  if ((id >> 3) >= a.xcd_chunk || w >= per_m * a.gy) return false;
  mblk = w / per_m;
  const int rest = w - mblk * per_m;
  b = rest / a.gx;
  tile_n = rest - b * a.gx;
  return true;
}

}  // namespace dmel
