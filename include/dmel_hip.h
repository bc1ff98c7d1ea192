/*
 * dmel_hip.h -- C ABI of libdmel_hip.so, the MI355X (gfx950) native dMel codec hot path.
 *
 * Drop-in boundary: the reference's plugin surface is its Python module API
 * (Hydra `_target_` strings); its one native ABI is `fwd_cuda` of the anti-alias activation
 * (models/modules/bigvgan/alias_free_activation/cuda/anti_alias_activation_cuda.cu:212,
 *  anti_alias_activation.cpp:21-23), a C++ (torch::Tensor) ABI.  This header is what a binding of the
 * reference's path binds instead: plain pointers, sizes and an opaque stream -- no torch types.
 *
 * Conventions
 *   - every `const float*`/`float*` tensor argument is DEVICE memory unless the name ends in `_host`;
 *   - the caller owns every buffer, including the workspace (size from the matching *_workspace_bytes);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all launches are asynchronous on
 *     it and the library never synchronises inside a forward call;
 *   - return value: 0 = ok, <0 = invalid argument / unsupported configuration, >0 = hipError_t;
 *     dmel_last_error() returns a thread-local description of the last failure;
 *   - layouts are the reference's: activations (B, C, T) fp32 with T contiguous, audio (B, L) fp32,
 *     token ids (B, G*R, T4) int32.
 */
#ifndef DMEL_HIP_H
#define DMEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMEL_OK 0
#define DMEL_EINVAL (-1)
#define DMEL_EUNSUPPORTED (-2)
#define DMEL_EMISSING (-3)

/* Arithmetic of the convolutions of a handle (dmel_*_set_precision).  Tensors are fp32 in HBM in every mode.
 *  FP32 (default, the parity path): fp32-grade products, fp32 accumulation; results within 1e-4 of the reference run in
 *      fp32.  The library is free to form the products either on the fp32 MFMA or from an exact three-way bf16 split of
 *      both operands on the bf16 matrix cores (six partial products, dropped terms < 2^-21 relative; DESIGN.md "split
 *      fp32") -- both meet the same error bound against an fp64 evaluation and tests hold them to it.
 *  FP32_MFMA: force the native v_mfma_f32_32x32x2_f32 kernel (every product one exact fp32 fma).
 *  FP32_F16X2: fp32-grade products from a TWO-way fp16 split of both operands (a = a_hi + 2^-11 a_lo, a_hi = fp16(a) round to nearest,
 *      a_lo = fp16((a - a_hi) 2^11): 22 significant bits, |a - (a_hi + 2^-11 a_lo)| <= 2^-22 |a|, against the 24 of fp32) and THREE partial products on the fp16 matrix
 *      cores (a_hi b_hi into one fp32 accumulator, a_hi b_lo + a_lo b_hi into a second one that is folded in with 2^-11 at the end; the
 *      dropped a_lo b_lo is < 2^-22 |ab|): the "3xTF32" construction with fp16 pieces (same 22 bits), whose errors are random in sign and
 *      vanish under the rounding of a K ~ 10^3 fp32 accumulation -- half the matrix-core time of the six-product
 *      bf16 split for the same error against an fp64 evaluation (tests hold both to the same bound).  Inputs are staged as x 2^-6 and
 *      the weight image carries 2^6, so the fp16 range covers |x| < 4.19e6 (larger magnitudes overflow to inf -- loudly) and values
 *      below 2^-8 keep an ABSOLUTE error of 2^-30: use it for activations, not for back-propagated gradients.
 *      DOMAIN, stated once more because inference launches do not rescale their inputs (training launches over gradients do):
 *          |x| < 4.19e6 (= 2^6 * 65504), relative error 2^-22 for |x| >= 2^-8 = 3.9e-3, absolute error <= 2^-30 = 9.3e-10 below that
 *          (0.5 % of a 1e-7 input, 7e-5 of a 1e-5 one: tests/test_gpu_parity.py::test_f16_split_conv_over_the_magnitude_range).
 *      Audio-network activations (|x| ~ 1e-3 .. 1e2) sit inside it.  DMEL_DEBUG_F16_RANGE=1 makes every such launch reduce max |x| of
 *      its input, synchronise and FAIL if the bound is exceeded (a debugging aid: it serialises the stream).  The vocoder handle
 *      selects it by default (DMEL_PRECISION_FP32 there means "fp32-grade, library's choice"); WaveNet handles keep the six-product
 *      split unless asked, because the encoder's token ids are defined by it.  Training entry points choose per launch: the six-product split wherever a gradient
 *      tensor is an operand as it is, the fp16 split where the operand is an activation (discriminator / decoder forward) or a gradient
 *      tensor the library first scales by its own maximum (the discriminator's backward-data and long-row weight gradients: a reduction on
 *      the same stream finds max |dy|, the kernel stages dy x 2^(13 - exponent)).
 *      Single-segment launches (one input, unit input stride: the vocoder's AMP-block convolutions, 1x1 projections) run a form of the
 *      kernel whose tap count is compiled in; it computes the same bits as the generic form.  DMEL_CONV_SPEC=0 (read per launch) sends
 *      every launch to the generic form, for A/B timing and bit-identity tests.
 *  FP32_BF16X3: force the six-product bf16 split where FP32 would pick the fp16 one.
 *  BF16: opt-in throughput mode, the library-side equivalent of running the reference's codec under dtype: bfloat16
 *      (config/lm/lm_config.yaml:1,83; models/lm_lit_modules.py:52-55): weights and staged activations rounded to bf16
 *      (nearest-even), fp32 accumulation; activations, biases, residuals and the quantizer stay fp32.  More accurate than
 *      the reference's bf16 autocast, but NOT within the 1e-4 bar. */
#define DMEL_PRECISION_FP32 0
#define DMEL_PRECISION_BF16 1
#define DMEL_PRECISION_FP32_MFMA 2
#define DMEL_PRECISION_FP32_F16X2 3
#define DMEL_PRECISION_FP32_BF16X3 4

const char* dmel_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int dmel_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * STFT -> magnitude -> mel -> log            replaces utils/spectrogram.py:41-81 (LinearSpectrogram.forward)
 * The plan caches the hann window, FFT twiddles and the sparse Slaney mel basis on the device, as the
 * reference caches mel basis + window per (config, device) (utils/spectrogram.py:43-56).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmel_stft_plan dmel_stft_plan;

/* f_max <= 0 means sample_rate/2 (librosa default when fmax=None).  window_host: win_length floats or
 * NULL for the periodic hann window torch.hann_window(win_length) (spectrogram.py:53).
 * Supported: n_fft in {512, 1024, 2048}, win_length <= n_fft, (n_fft - hop_length) even, n_mels <= 128. */
int dmel_stft_plan_create(dmel_stft_plan** plan, int sample_rate, int n_fft, int win_length, int hop_length,
                          int n_mels, double f_min, double f_max, const float* window_host);
void dmel_stft_plan_destroy(dmel_stft_plan* plan);
/* Host-only helper (no device needed): the dense (n_mels, n_fft/2+1) Slaney mel basis, librosa 0.10.2
 * filters.mel(htk=False, norm="slaney") semantics (call site utils/spectrogram.py:45-52).  f_max <= 0: sr/2. */
int dmel_mel_basis_host(int sample_rate, int n_fft, int n_mels, double f_min, double f_max, float* basis_host);
/* Copy the dense (n_mels, n_fft/2+1) mel basis the plan was built from to host memory. */
int dmel_stft_plan_mel_basis(const dmel_stft_plan* plan, float* basis_host);
/* Number of frames for an L-sample clip: 1 + (L + 2*pad - n_fft) / hop with pad = (n_fft-hop)/2. */
int64_t dmel_stft_num_frames(const dmel_stft_plan* plan, int64_t L);
/* audio (B, L) with row stride audio_row_stride (elements).  out (B, n_mels, T).
 * lengths: NULL, or B int64 sample counts: frames t >= lengths[b]/hop are written as 0 (the `mels * mask`
 * of codec_lit_modules.py:492-506 fused in). */
int dmel_stft_logmel_f32(const dmel_stft_plan* plan, const float* audio, int64_t audio_row_stride,
                         const int64_t* lengths, float* out, int B, int64_t L, void* stream);

/* Several streams on one GPU (round 3; dmel_codec_amd.pipeline.CodecLanes sets it): on != 0 makes every later STFT launch of the process ask for
 * 152 KB of LDS, i.e. one workgroup per CU and no room beside it for a workgroup of the convolution kernels.  Launched from different
 * streams, the two kinds of workgroup otherwise end up on one CU, and 3-11 % of the STFT launches then return one wrong frame (measured,
 * mechanism not understood: csrc/stft_logmel.hip, profiles/r03_stft_concurrency.txt).  No reference counterpart (utils/spectrogram.py:58-79 is
 * one torch.stft call on the current stream).  Costs nothing at the codec's sizes (<= 256 workgroups), 2.5x at 256 x 60 s. */
int dmel_stft_set_exclusive_cu(int on);
/* The same launch with the linear magnitudes sqrt(re^2 + im^2 + 1e-9) (utils/spectrogram.py:76) as a second, optional output:
 * linear (B, T, n_fft/2 + 1), frame-major so that every frame is one coalesced row; logmel_out may be NULL (then the mel stage is
 * skipped).  Consumer: the multi-resolution STFT loss BASELINE.json's north_star names (absent from the reference). */
int dmel_stft_f32(const dmel_stft_plan* plan, const float* audio, int64_t audio_row_stride, const int64_t* lengths,
                  float* logmel_out /*nullable*/, float* linear_out /*nullable*/, int B, int64_t L, void* stream);
/* The frames of a WINDOW of a longer signal (streaming encode; the reference frames a finished clip once, utils/spectrogram.py:58-79):
 * audio (B, n_samples) holds the absolute samples [s0, s0 + n_samples) of a stream; the call writes the absolute frames
 * [first_frame, first_frame + n_frames) to logmel_out (B, n_mels, n_frames) / linear_out (B, n_frames, n_fft/2 + 1).  total_length is
 * the length of the whole signal, or < 0 while it is not known yet.  Reflection happens only where the signal itself starts (absolute
 * sample 0) and, once the length is known, where it ends; every frame has the bits dmel_stft_logmel_f32 gives it on the whole clip (same
 * kernel, same per-frame arithmetic).  lengths: as above, in absolute samples (frames t >= lengths[b]/hop are written as 0).  Every
 * sample the frames read -- frame t reads [t*hop - pad, t*hop - pad + n_fft), reflected at the ends -- must lie in the buffer (checked). */
int dmel_stft_window_f32(const dmel_stft_plan* plan, const float* audio, int64_t audio_row_stride, int64_t n_samples, int64_t s0,
                         const int64_t* lengths, float* logmel_out /*nullable*/, float* linear_out /*nullable*/, int B,
                         int64_t first_frame, int64_t n_frames, int64_t total_length, void* stream);
/* The same launch for B INDEPENDENT streams (a pool of live encode sessions: every microphone starts, stalls and ends on its own):
 * s0, n_valid, first_frame, n_frames, total_length are HOST tables of B entries.  audio (B, n_samples) is one buffer width; row b holds
 * the absolute samples [s0[b], s0[b] + n_valid[b]) of stream b, n_valid[b] <= n_samples (n_valid == NULL: n_samples for every item).
 * Item b's frames [first_frame[b], first_frame[b] + n_frames[b]) go to the first n_frames[b] columns of its rows of logmel_out
 * (B, n_mels, Tmax) / linear_out (B, Tmax, n_fft/2 + 1), Tmax = max n_frames; the columns behind them are NOT written.  n_frames[b] == 0
 * is an idle item: nothing of it is read or written (and nothing is launched when every item is idle).  Every item is checked by the
 * rules of dmel_stft_window_f32 against its own [s0[b], s0[b] + n_valid[b]); a failure is DMEL_EINVAL, names the item, and nothing is
 * launched.  Same kernel body, same per-frame arithmetic: a frame has the bits dmel_stft_window_f32 gives it.  lengths: device, as above.
 * table_scratch: device memory for 4 B int64 (the per-item windows as the kernel reads them).  The host tables are copied as launch
 * arguments: the caller may overwrite them as soon as the call returns.  dmel_stft_set_exclusive_cu applies as to every STFT launch. */
int dmel_stft_window_items_f32(const dmel_stft_plan* plan, const float* audio, int64_t audio_row_stride, int64_t n_samples,
                               const int64_t* s0, const int64_t* n_valid /*nullable*/, const int64_t* lengths /*nullable*/,
                               float* logmel_out /*nullable*/, float* linear_out /*nullable*/, int B, const int64_t* first_frame,
                               const int64_t* n_frames, const int64_t* total_length, int64_t* table_scratch, void* stream);

/* Backward of the linear magnitudes of dmel_stft_f32 -- what turns the multi-resolution STFT loss BASELINE.json's north_star names into a
 * LOSS (the reference has neither; its STFT framing is utils/spectrogram.py:58-76).  grad_linear (B, T, n_fft/2 + 1) = dL/d|S|, frame-major
 * like linear_out; daudio (B, L) is overwritten with dL/daudio.  The handle holds the windowed DFT matrix and its transpose in MFMA tile
 * order: both transforms run as GEMMs on the library's convolution kernel (split-fp32 arithmetic), followed by an overlap-add that folds
 * the reflect padding back.  n_fft any multiple of 16 up to 4096 (the forward kernel: 512 / 1024 / 2048). */
typedef struct dmel_stft_grad dmel_stft_grad;
int dmel_stft_grad_create(dmel_stft_grad** out, int n_fft, int win_length, int hop_length, const float* window_host /*nullable: periodic hann*/);
void dmel_stft_grad_destroy(dmel_stft_grad* h);
size_t dmel_stft_grad_workspace_bytes(const dmel_stft_grad* h, int B, int64_t L);
int dmel_stft_magnitude_backward_f32(const dmel_stft_grad* h, const float* audio, int64_t audio_row_stride, const float* grad_linear,
                                     float* daudio, int64_t daudio_row_stride, int B, int64_t L, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sample-rate conversion in front of the STFT    replaces torchaudio.functional.resample as called by
 * LogMelSpectrogram.forward(x, sample_rate=...) (utils/spectrogram.py:122-123): polyphase windowed-sinc filter bank,
 * y[b, n * new + p] = sum_k bank[p][k] * xpad[b, n * orig + k], orig_freq / new_freq already divided by their gcd, xpad = x with `width`
 * zeros in front, kw = 2 * width + orig_freq taps per phase.  filter_bank_dev: (new_freq, kw) fp32 on the device (the caller builds it:
 * it depends on torchaudio's rolloff / window choices, which are host-side policy); x (B, L), y (B, Lout), Lout <= ceil(new * L / orig).
 * ---------------------------------------------------------------------------------------------- */
int dmel_resample_f32(const float* x, float* y, const float* filter_bank_dev, int B, int64_t L, int64_t Lout, int orig_freq,
                      int new_freq, int width, void* stream);
/* The outputs of a WINDOW of a longer signal (streaming at the sound card's rate; the reference resamples a finished clip once,
 * utils/spectrogram.py:122-123): x (B, n_samples), rows x_row_stride floats apart, holds the absolute input samples [s0, s0 + n_samples)
 * of a stream; the call writes the absolute output samples [o0, o0 + n_out) to y (B, n_out).  o0 may be any value, not only a multiple
 * of new_freq.  total_length is the length of the whole input, or < 0 while it is not known yet.  Zero padding happens only where the
 * signal itself starts (absolute sample < 0) and, once the length is known, where it ends (>= total_length); every output has the bits
 * dmel_resample_f32 gives it on the whole clip (same kernel, same tap loop).  filter_bank_dev, orig_freq, new_freq, width: as above.
 * Every sample the outputs read -- output o reads [(o / new) * orig - width, (o / new) * orig + width + orig) -- must lie in the buffer
 * or in the zero padding (checked: DMEL_EINVAL, nothing is launched, y is left as it was). */
int dmel_resample_window_f32(const float* x, int64_t x_row_stride, int64_t n_samples, int64_t s0, float* y, const float* filter_bank_dev,
                             int B, int64_t o0, int64_t n_out, int64_t total_length, int orig_freq, int new_freq, int width, void* stream);
/* The same launch for B INDEPENDENT streams, EACH WITH ITS OWN RATE PAIR (a pool of live sessions whose sound cards run at 48, 44.1
 * and 16 kHz): ONE launch converts all of them.  s0, n_valid, y_off, rate_index, o0, n_out, total_length are HOST tables of B entries,
 * rates a HOST table of n_rates descriptors of four int64: (bank_off, orig_freq, new_freq, width), the rates divided by their gcd, the
 * bank of that pair -- (new_freq, 2 * width + orig_freq) fp32, as above -- at bank_arena_dev + bank_off (checked to lie inside the
 * arena of bank_arena_floats floats).  x (B, n_samples) is one buffer width, rows x_row_stride floats apart; row b holds the absolute
 * samples [s0[b], s0[b] + n_valid[b]) of stream b, n_valid[b] <= n_samples, at rate rates[rate_index[b]].  Item b's outputs
 * [o0[b], o0[b] + n_out[b]) go to y + b * y_row_stride + y_off[b]; NOTHING ELSE of y is written, so y may be rows that already hold
 * data in front of y_off[b] (a pool lets the launch write straight behind a slot's carried sample tail).  n_out[b] == 0 is an idle
 * item: nothing of it is read, checked or written (and nothing is launched, DMEL_OK, when every item is idle).  Every other item is
 * checked by the rules of dmel_resample_window_f32 against its own [s0[b], s0[b] + n_valid[b]) and its own rate, and
 * y_off[b] + n_out[b] <= y_row_stride; a failure is DMEL_EINVAL, names the item, nothing is launched and y is left as it was.  Same
 * kernel text, same tap loop: an output has the bits dmel_resample_f32 gives it on the whole clip.  A workgroup stages ITS item's bank
 * in LDS when it has at most 15 K floats and reads it from the arena otherwise (44.1 -> 48 kHz: 160 x 161); a workgroup behind its
 * item's last output leaves before either.  Grid (ceil(max n_out / 256), B).
 * table_scratch: device memory for 7 B + 4 n_rates int64 (the items and rates as the kernel reads them).  The host tables are copied as
 * launch arguments: the caller may overwrite them as soon as the call returns. */
int dmel_resample_window_items_f32(const float* x, int64_t x_row_stride, int64_t n_samples, const int64_t* s0, const int64_t* n_valid,
                                   float* y, int64_t y_row_stride, const int64_t* y_off, const float* bank_arena_dev,
                                   int64_t bank_arena_floats, const int64_t* rates, int n_rates, const int64_t* rate_index, int B,
                                   const int64_t* o0, const int64_t* n_out, const int64_t* total_length, int64_t* table_scratch,
                                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * The sample format of the wire: 16-bit signed PCM or 8-bit G.711 (mu-law, A-law) <-> fp32, B ragged convert-copies in ONE launch (a pool of live sessions whose
 * microphones, RTP streams and sound cards carry int16; no reference counterpart: the reference reads finished float clips).
 * src, src_fmt, dst, dst_fmt, n are HOST tables of B entries; src[b] / dst[b] are DEVICE pointers to n[b] samples of format
 * src_fmt[b] / dst_fmt[b].  Item b:
 *   s16 -> f32   y = (float)x * 2^-15: exact; full scale is -1.0 and the largest value 1 - 2^-15.
 *   f32 -> s16   y = rne(clamp(x * 32768, -32768, 32767)): the product is exact (a power of two), rne is round to nearest, ties to
 *                EVEN (v_rndne_f32; not the current rounding mode, not truncation, not half away from zero): 0.5 / 32768 -> 0,
 *                1.5 / 32768 -> 2, 2.5 / 32768 -> 2.  NaN -> 0, +-inf saturate, no dither: the result is deterministic.
 *   f32 -> f32   the words copied untouched (a pool with mixed sessions still makes one launch).
 *   s16 -> s16   refused.
 * G.711, the wire of telephony (8-bit mu-law or A-law; RTP payload types 0 and 8): the rule of ITU-T G.711 as Sun's g711.c and CPython's
 * audioop restate it, on the s16 value x, >> an arithmetic shift, every comparison of it an equality of bits:
 *   mu-law encode   v = x >> 2; neg = v < 0; m = min((neg ? -v : v) + 33, 8191); seg = floor(log2 m) - 5  (0 .. 7);
 *                   code = ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ (neg ? 0x7F : 0xFF)
 *   mu-law decode   u = ~code & 0xFF; t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4); x = (u & 0x80) ? 0x84 - t : t - 0x84
 *   A-law encode    v = x >> 3; neg = v < 0; m = neg ? -v - 1 : v; seg = max(floor(log2 max(m, 1)) - 4, 0);
 *                   mant = seg < 2 ? (m >> 1) & 15 : (m >> seg) & 15; code = ((seg << 4) | mant) ^ (neg ? 0x55 : 0xD5)
 *   A-law decode    a = code ^ 0x55; t = (a & 15) << 4; seg = (a & 0x70) >> 4; t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
 *                   x = (a & 0x80) ? t : -t
 *   law -> f32   y = decode(code) * 2^-15: exact.
 *   f32 -> law   code = encode(the f32 -> s16 rule above, unchanged): NaN and 0.0 give 0xFF (mu-law) and 0xD5 (A-law).
 *   law <-> s16 and law <-> law are refused: not conversions served here.
 * encode(decode(c)) == c for all 256 A-law codes and for every mu-law code but 0x7F ("negative zero": decodes to 0, encodes as 0xFF).
 * The segment is a count of leading zeros, so every lane runs the same instructions whatever its sample.
 * Format codes 2 .. 7 and codes above 9 are not assigned and are refused.
 * n[b] == 0 is an idle item: its pointers are not looked at, nothing of it is read or written (and nothing is launched, DMEL_OK, when
 * every item is idle).  Checked before anything is launched -- a failure is DMEL_EINVAL, names the item, and leaves every destination
 * as it was: 1 <= B <= 65535, formats in range, n[b] >= 0, non-NULL pointers where n[b] > 0, an s16 pointer 2-byte and an f32
 * pointer 4-byte aligned (a law pointer needs no alignment).  NOT checked: that no destination overlaps a source or another
 * destination (the caller's to guarantee).
 * Grid (ceil(max n / 2048), B); a workgroup behind its item's last sample leaves at once.  An item whose src AND dst are 16-byte
 * aligned moves whole groups of 8 samples with 16-byte loads and stores -- a law item whose f32 pointer is 16-byte and whose law pointer
 * is 8-byte aligned, with one 8-byte access on the law side and two 16-byte ones on the f32 side -- any other item goes sample by
 * sample: same arithmetic, same bits.  table_scratch: device memory for 4 B int64, 8-byte aligned (the items as the kernel reads them).  The host tables are
 * copied as launch arguments: the caller may overwrite them as soon as the call returns.
 * ---------------------------------------------------------------------------------------------- */
#define DMEL_SAMPLE_F32 0
#define DMEL_SAMPLE_S16 1
#define DMEL_SAMPLE_ULAW 8 /* the 8-bit formats start at 8 */
#define DMEL_SAMPLE_ALAW 9
int dmel_pcm_convert_items(const void* const* src, const int32_t* src_fmt, void* const* dst, const int32_t* dst_fmt, const int64_t* n,
                           int B, void* table_scratch, void* stream);
/* The same launch with INTERLEAVED CHANNELS (the codec is mono; sound cards, WAV, RTP L16 and WebRTC deliver interleaved frames, usually
 * stereo, and a playback device opened as stereo wants them).  An interleaved piece of n frames and c channels is a contiguous (n, c)
 * array: frame i, channel j is element i * c + j; 1 <= c <= DMEL_MAX_CHANNELS (8).  n[b] counts FRAMES.  src_ch / dst_ch: int32 HOST
 * tables of the channel counts (NULL: all 1); src_pick: NULL, or per item -1 (the mean) or a channel 0 .. src_ch - 1.  Item b:
 *   downmix (c -> 1)   each channel's sample goes to f32 by its format's rule above (s16: x / 32768; law: decode / 32768; f32: the value
 *                      itself); then acc = x_0; acc += x_1; ... acc += x_{c-1} in fp32, in channel order; then y = acc / (float)c, the
 *                      IEEE correctly rounded fp32 division -- NOT a multiply by a rounded reciprocal.  Bit for bit numpy.mean(y, axis=0)
 *                      of the channel-first float32 array, which is what librosa's to_mono computes (the reference loads its clips with
 *                      librosa.load(..., mono=True): dataset/lhotse_tts_dataset.py:29-30, evaluation/evaluation_utils.py:215-224).  For
 *                      s16 and law sources the channel values and their sum are exact in fp32 (at most 16 + 3 bits), so the result is the
 *                      fp64 mean rounded once.  Nothing is sanitised: an f32 NaN or inf propagates as in a mono f32 item.
 *   pick (c -> 1, k)   y = x_k by its format's rule, no arithmetic; for f32 the word is untouched.
 *   fan-out (1 -> c)   the mono sample is converted ONCE by the f32 -> format rule above and stored c times, frame by frame; for
 *                      f32 -> f32 the word is copied.
 * The rule that one side of every item is f32 holds unchanged (stereo s16 -> mono s16 is refused like s16 -> s16).  Refused as well,
 * before anything is launched, DMEL_EINVAL naming the item: a channel count outside 1 .. 8; both counts of an item above 1; a pick
 * outside the source's channels or given with src_ch == 1.  Not served at all: weights, channel maps, planar (channel-first) pieces.
 * Pointers are aligned to the sample size as before; n[b] * c < 2^40.  With every count 1 and no pick this IS dmel_pcm_convert_items
 * (which calls it with NULL tables): the items' table words, the code path and the bits are the same.
 * A workgroup owns 2048 frames of its item.  A stereo item (c == 2) whose src AND dst are 16-byte aligned moves a thread's 8 consecutive
 * frames -- 8 mono elements on one side, 16 channel samples on the other -- with 16-byte loads and stores; any other channel count, an
 * unaligned item and the frames behind the last whole 8 go frame by frame: same functions, same bits.  The channel counts and the pick
 * ride in spare bits of the item's fourth table word: table_scratch stays 4 B int64. */
#define DMEL_MAX_CHANNELS 8
int dmel_pcm_convert_items_ch(const void* const* src, const int32_t* src_fmt, const int32_t* src_ch, const int32_t* src_pick,
                              void* const* dst, const int32_t* dst_fmt, const int32_t* dst_ch, const int64_t* n, int B,
                              void* table_scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data front end on the GPU: what LhotseTTSDataset.__getitem__ + collate_fn do to the decoded clips of
 * a batch (dataset/lhotse_tts_dataset.py:29-32, :46-65): every clip peak-normalised, `librosa.util.normalize(audio) * 0.95` =
 * x / max|x| * peak (a clip whose peak is below the smallest normal float is left unscaled, as librosa does), right-padded with zeros
 * to Lmax and stacked: audios (B, 1, Lmax) f32, audio_lengths (1, B) int32.  clips_dev: B device pointers (device array) to the mono
 * clips where the decoder / resampler left them; lengths_dev: their sample counts (device, int64); order_dev (nullable, device int32):
 * output row b takes clip order[b] (the reference sorts a batch longest-first on the host, :20); peaks_scratch: B words.
 * ---------------------------------------------------------------------------------------------- */
int dmel_collate_peak_f32(const float* const* clips_dev, const int64_t* lengths_dev, const int32_t* order_dev /*nullable*/, float* audios,
                          int32_t* audio_lengths, uint32_t* peaks_scratch, int B, int64_t Lmax, float peak, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Anti-aliased Snake / SnakeBeta           replaces fwd_cuda (anti_alias_activation_cuda.cu:212-246) and the
 * torch Activation1d (alias_free_activation/torch/act.py:25-30): x2 up (12-tap kaiser-sinc, replicate pad)
 * -> x + 1/(b+1e-9) sin^2(a x) -> x2 down (12 taps, replicate pad 5/6).  alpha/beta: (C) as stored in the
 * state dict; logscale != 0 applies exp() as the reference does.  beta == NULL means Snake (beta := alpha).
 * up_filter12_host / down_filter12_host: the 12 taps of UpSample1d.filter and DownSample1d.lowpass.filter (host pointers; they
 * become launch constants) -- the two arguments of fwd_cuda(input, up_filter, down_filter, alpha, beta)
 * (anti_alias_activation.cpp:19-23); the reference registers the same kaiser-sinc taps for both.
 * ---------------------------------------------------------------------------------------------- */
int dmel_aa_snake_f32(const float* x, float* y, const float* alpha, const float* beta, const float* up_filter12_host,
                      const float* down_filter12_host, int logscale, int B, int C, int64_t T, void* stream);
/* The same over ITEMS of different lengths in one launch (extension; the reference pads a batch and activates the padding): x, y
 * (B, C, T) with T the row PITCH, lengths_dev (B) device int64, 0 <= lengths[b] <= T (clamped into that range on the device).  Item b
 * is a row of lengths[b] columns: its replicate padding ends at column lengths[b] - 1, y[b, :, :lengths[b]] is BIT-IDENTICAL to
 * dmel_aa_snake_f32 on x[b:b+1, :, :lengths[b]], and nothing at or beyond column lengths[b] of a row is read or written (an item of
 * length 0 is left alone).  No host read of the lengths, no synchronisation. */
int dmel_aa_snake_items_f32(const float* x, float* y, const float* alpha, const float* beta, const float* up_filter12_host,
                            const float* down_filter12_host, int logscale, int B, int C, int64_t T, const int64_t* lengths_dev,
                            void* stream);
/* Three activations of ONE tensor in one launch (extension: the three AMP blocks behind an up-sampler of BigVGAN each begin with an
 * activation of the same tensor, bigvgan/bigvgan.py:376-382): y_k = activation(x; alpha_k, beta_k), k = 0..2.  x is read and up-filtered
 * once; every y_k is BIT-IDENTICAL to dmel_aa_snake_f32 (dmel_aa_snake_items_f32 for the items form, same contract: columns at or beyond
 * lengths[b] are neither read nor written) with its parameters.  beta_k NULL = Snake.  x and the three outputs must be distinct
 * buffers; each output takes 16-byte stores when it, x and the rows (T % 4 == 0) are 16-byte aligned, dword stores otherwise. */
int dmel_aa_snake3_forward(const float* x, float* y0, float* y1, float* y2, const float* alpha0, const float* beta0, const float* alpha1,
                           const float* beta1, const float* alpha2, const float* beta2, const float* up_filter12_host,
                           const float* down_filter12_host, int logscale, int B, int C, int64_t T, void* stream);
int dmel_aa_snake3_forward_items(const float* x, float* y0, float* y1, float* y2, const float* alpha0, const float* beta0,
                                 const float* alpha1, const float* beta1, const float* alpha2, const float* beta2,
                                 const float* up_filter12_host, const float* down_filter12_host, int logscale, int B, int C, int64_t T,
                                 const int64_t* lengths_dev, void* stream);
/* The vocoder's tail in one launch (extension): y (B, 1, T) = act(conv_post(activation(x))), BIT-IDENTICAL to dmel_aa_snake_f32 followed
 * by dmel_conv_post_f32 (the items form: to dmel_aa_snake_items_f32 followed by dmel_conv_post_items_f32, y[b, 0, lengths[b]:] = 0); the
 * activated (B, C, T) tensor is never written.  Arguments as in those two; K odd, at most 257 taps. */
int dmel_snake_post_forward(const float* x, const float* alpha, const float* beta, const float* up_filter12_host,
                            const float* down_filter12_host, int logscale, const float* w_dev, float bias, int act, float* y, int B, int C,
                            int K, int64_t T, void* stream);
int dmel_snake_post_forward_items(const float* x, const float* alpha, const float* beta, const float* up_filter12_host,
                                  const float* down_filter12_host, int logscale, const float* w_dev, float bias, int act, float* y, int B,
                                  int C, int K, int64_t T, const int64_t* lengths_dev, void* stream);
/* Backward of dmel_aa_snake_f32 (the reference's fused kernel has none: alias_free_activation/cuda/activation1d.py:29-32;
 * SURVEY.md section 8(f) rank 1, C-ABI row `aa_snake(+_bwd)`): dx (B, C, T), dalpha (C), dbeta (C; NULL exactly when beta is NULL,
 * i.e. Snake, whose single parameter then receives both contributions).  Gradients are with respect to the STORED parameters
 * (the log-scale ones when logscale != 0).  dalpha / dbeta are overwritten.  Summation order is not fixed (atomics). */
int dmel_aa_snake_backward_f32(const float* x, const float* dy, float* dx, const float* alpha, const float* beta /*nullable*/,
                               float* dalpha, float* dbeta /*nullable*/, const float* up_filter12_host,
                               const float* down_filter12_host, int logscale, int B, int C, int64_t T, void* stream);

/* dx of the same backward alone, for frozen parameters (the vocoder under a waveform loss): no dalpha / dbeta reductions, memsets or
 * atomics; dx is BIT-IDENTICAL to dmel_aa_snake_backward_f32's.  add (B, C, T), nullable: dx = dx_act + add, the residual branch
 * x = xt + x of an AMP layer (bigvgan/bigvgan.py:132-141) without an add kernel of its own. */
int dmel_aa_snake_backward_input_f32(const float* x, const float* dy, const float* add /*nullable*/, float* dx, const float* alpha,
                                     const float* beta /*nullable*/, const float* up_filter12_host, const float* down_filter12_host,
                                     int logscale, int B, int C, int64_t T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Module handles.  Weights are handed over as HOST fp32 arrays under the reference's state-dict key names
 * (key names are part of the contract); the library folds weight norm (weight_g / weight_v),
 * re-tiles them for the MFMA kernels and uploads them.  *_finalize fails with DMEL_EMISSING when a required
 * key was never set.
 * ---------------------------------------------------------------------------------------------- */

/* WaveNet      replaces models/modules/wavenet.py:138-225 (forward :204-225, block :116-135) */
typedef struct dmel_wavenet dmel_wavenet;
int dmel_wavenet_create(dmel_wavenet** m, int input_channels /*0 = same as residual*/, int output_channels /*0 = none*/,
                        int residual_channels, int residual_layers, int dilation_cycle, int condition_channels /*0 = none*/);
void dmel_wavenet_destroy(dmel_wavenet* m);
int dmel_wavenet_set_precision(dmel_wavenet* m, int precision);   /* DMEL_PRECISION_*; may be changed between forwards */
int dmel_wavenet_set_tensor(dmel_wavenet* m, const char* key, const float* data_host, const int64_t* shape, int ndim);
int dmel_wavenet_finalize(dmel_wavenet* m);
size_t dmel_wavenet_workspace_bytes(const dmel_wavenet* m, int N, int64_t T);
/* x (N, Cin, T), condition (N, Ccond, T) or NULL, y (N, Cout, T).
 * in_lengths / out_lengths: NULL or N int64 frame counts; x is read as x * (t < in_lengths[n]) and y is
 * written as y * (t < out_lengths[n])  (the mask multiplies of codec_lit_modules.py:471-477,505-506).
 * group_repeat: lengths index = n / group_repeat (expand_mask, codec_lit_modules.py:156-157); with lengths given N must be a
 *   multiple of it (DMEL_EINVAL otherwise, nothing is written).
 * A length above T counts as T.  A length of 0 masks the whole item: an in_length of 0 feeds the stack zeros (y is then what the
 *   biases give), an out_length of 0 writes the item's y as zeros.  What stands in x at or behind in_lengths does not reach the
 *   result (1e30 there changes no bit).  The one-launch kernel and the layered path agree on all of this bit for bit
 *   (tests/test_gpu_wavenet_one_launch_matrix.py). */
int dmel_wavenet_forward(const dmel_wavenet* m, const float* x, const float* condition, float* y, int N, int64_t T,
                         const int64_t* in_lengths, const int64_t* out_lengths, int group_repeat,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Training path of the WaveNet (first module of SURVEY.md section 8(f) rank 1; C-ABI row `wavenet_block(+_bwd)`): what
 * `manual_backward(loss)` differentiates through autograd in the reference (codec_lit_modules.py:236,315 over
 * wavenet.py:116-135,204-225).  enable_training must precede finalize (the transposed weight images are packed there).
 * forward_train = forward without masks, keeping in `workspace` what backward needs; backward must be given the SAME
 * workspace, untouched, plus x / condition again.  Parameter gradients are written (overwritten) into one flat fp32 device
 * buffer of dmel_wavenet_grad_floats() elements; dmel_wavenet_grad_slot maps a state-dict key to its (offset, numel) there
 * (layout of each slot = the parameter's own layout).  dx / dcondition may be NULL when not needed.  Gradients are
 * fp32-grade regardless of the handle's precision. */
int dmel_wavenet_enable_training(dmel_wavenet* m, int on);
/* bf16 training mode (BASELINE config 3 "DDP bf16"; the reference switches dtype / Lightning precision, codec_lit_modules.py:52-56,
 * config/lm/lm_config.yaml:1,83): DMEL_PRECISION_BF16 makes every convolution of forward_train / backward run with operands rounded to
 * bf16 and fp32 accumulation -- forward, backward-data, and the weight gradients of rows of >= 256 samples (shorter rows keep the exact
 * fp32 kernel) -- while parameters, activations in HBM, gradients and the optimiser stay fp32 (autocast semantics).  The same setter
 * exists for the other three trainable handles.  Default DMEL_PRECISION_FP32 (the parity path). */
int dmel_wavenet_set_train_precision(dmel_wavenet* m, int precision);
/* Re-pack every weight image of a finalized handle from DEVICE tensors (after an optimiser step): keys / device_tensors
 * name the state-dict tensors (weights (Cout, Cin, k) and biases, contiguous fp32) as they currently live on the device.
 * Runs on `stream`, no host copy, no allocation; produces bit-identical images to set_tensor + finalize on the same values.
 * All or nothing: every key is resolved before the first copy or launch, a missing one is DMEL_EMISSING (named by dmel_last_error)
 * and leaves the handle as it was.  The same holds for the other two refresh entry points. */
int dmel_wavenet_refresh(dmel_wavenet* m, int n, const char* const* keys, const float* const* device_tensors, void* stream);
size_t dmel_wavenet_train_workspace_bytes(const dmel_wavenet* m, int N, int64_t T);
int64_t dmel_wavenet_grad_floats(const dmel_wavenet* m);
int dmel_wavenet_grad_slot(const dmel_wavenet* m, const char* key, int64_t* offset, int64_t* numel);
int dmel_wavenet_forward_train(const dmel_wavenet* m, const float* x, const float* condition, float* y, int N, int64_t T,
                               void* workspace, size_t workspace_bytes, void* stream);
int dmel_wavenet_backward(const dmel_wavenet* m, const float* x, const float* condition, const float* dy, float* dx /*nullable*/,
                          float* dcondition /*nullable*/, float* grads, int N, int64_t T, void* workspace, size_t workspace_bytes,
                          void* stream);
/* The exchange step of data-parallel training (the reference gets it from Lightning's DDP wrapper, config/codec/dMel_example.yaml:14:
 * gradient buckets are all-reduced while backward is still running).  dmel_wavenet_backward_hooked is dmel_wavenet_backward that calls
 * `on_ready(user, offset, numel)` on the calling host thread right after it has ENQUEUED the last kernel that writes
 * grads[offset, offset + numel): first the tail (skip_projection + output_projection), then residual_layers L-1 ... 0 (one contiguous
 * region per block: the bucket SURVEY section 8(e) asks for), then input_projection.  The regions are disjoint and cover the whole
 * buffer.  A caller that records an event on `stream` inside the callback and lets a communication stream wait for it overlaps the
 * all-reduce of block k with the backward of blocks k-1 ... 0.  on_ready == NULL: plain dmel_wavenet_backward. */
typedef void (*dmel_grad_ready_fn)(void* user, int64_t offset, int64_t numel);
int dmel_wavenet_backward_hooked(const dmel_wavenet* m, const float* x, const float* condition, const float* dy, float* dx /*nullable*/,
                                 float* dcondition /*nullable*/, float* grads, int N, int64_t T, void* workspace,
                                 size_t workspace_bytes, void* stream, dmel_grad_ready_fn on_ready, void* user);

/* Incremental (streaming) forward with state carry -- SURVEY.md section 8(f) rank 2: the LM emits tokens, the codec decodes while it
 * does (the reference decodes once at the end, models/lm_lit_modules.py:467-471).  Every block is a "same"-padded convolution, so block
 * l's output at time t needs block l-1's output up to t + dilation_l: instead of re-running a halo of old frames through the stack for
 * every chunk, the caller keeps the OUTPUT HISTORY of every block and each step only computes the new columns of every block.
 *   hist (L + 1, N, C, cap): hist[0] = the (masked) input x_0 (after input_projection, when the model has one: not supported here),
 *                            hist[l] = output of block l; time axis in window coordinates [0, cap)
 *   skip (N, C, cap): running sum of the blocks' skip outputs;  cond (N, Ccond, cap) or NULL;  y (N, Cout, cap)
 *   prev[l], next[l], l = 0..L: columns [0, prev[l]) of level l are already valid; the call makes [prev[l], next[l]) valid.
 *     next[0] = how far x_0 / cond have been written by the caller; mid-stream next[l] <= next[l-1] - dilation_l (checked);
 *     at the end of the sequence next[l] = next[0] = total length for every l (zero padding past the end, like the whole-sequence call).
 *   y gets columns [prev[L], next[L]).  scratch: N * 2 C * cap floats.
 * Numerically identical to dmel_wavenet_forward column by column (same kernels, same reduction order). */
int dmel_wavenet_stream_step(const dmel_wavenet* m, float* hist, float* skip, const float* cond /*nullable*/, float* y, float* scratch,
                             int N, int64_t cap, const int64_t* prev, const int64_t* next, void* stream);
/* The same step for stacks WITH an input projection and with the output mask -- the encoder side of a live conversation: audio chunks
 * in, token ids out, equal to encode() (replaces, incrementally, codec_lit_modules.py:462-466, 486-513 over wavenet.py:204-225).
 *   x (N, Cin, cap), given exactly when the model has an input projection: the raw input in the same window coordinates; the call fills
 *     hist[0][:, :, prev[0]:next[0]] = silu(input_projection(x)) (wavenet.py:205-207).  Without one the caller writes hist[0] as above.
 *   out_lengths (N / group_repeat,) or NULL, relative to column 0: y columns at or behind it are written as 0 (the output mask of
 *     dmel_wavenet_forward, codec_lit_modules.py:505-506).
 *   origin: the absolute frame held in column 0.  origin > 0 declares that column 0 is NOT the start of the sequence: a step whose
 *     windows would reach in front of it (prev[l] < dilation_l with new columns on level l) is refused instead of reading zero padding.
 *   scratch: N * 2 C * cap floats followed by N int64.
 * Narrow unconditioned stacks (the conditions of the whole-sequence kernel: residual channels in (32, 80], no condition, no output
 * projection, dilations <= 8, DMEL_PRECISION_FP32) run the step as ONE launch (csrc/wavenet_stream.hip), cut into sub-steps of at most 96
 * new columns per level; everything else, and every call under DMEL_WAVENET_STREAM_FUSED=0, runs the layered step.  Both produce the
 * bits of dmel_wavenet_forward column by column.  Measured at 30 new frames per push, 70 channels (profiles/stream_encode.txt): a whole
 * push 0.69 against 1.02 ms at 8 items, 0.71 against 1.10 ms at 128 items -- hence the default at every batch size. */
int dmel_wavenet_stream_step_ex(const dmel_wavenet* m, const float* x /*nullable*/, float* hist, float* skip, const float* cond /*nullable*/,
                                float* y, float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                const int64_t* out_lengths /*nullable*/, int group_repeat, int64_t origin, void* stream);
/* The same step with PER-UTTERANCE frontiers -- independent live sessions in one launch: item n belongs to utterance n / group_repeat
 * (N % group_repeat == 0), and prev, next (N / group_repeat, L + 1) and origin (N / group_repeat) are HOST tables with one row per
 * utterance, each in the window coordinates of that utterance's own column 0; out_lengths stays per utterance and relative to that
 * column 0.  A row with next == prev on every level is an IDLE item: its workgroups write nothing to hist, skip or y.  Every row is
 * checked on the host by the rules of dmel_wavenet_stream_step_ex (frontier order, no window in front of an origin > 0, ranges within
 * cap); a bad row is DMEL_EINVAL, dmel_last_error names the utterance, and nothing is launched.  A row may carry any number of new
 * columns: the step is cut into sub-steps of at most 96 new columns per level, as many as the longest row needs, and a row that is done
 * early is idle in the later ones.  Only the stacks of the one-launch kernel are taken (residual channels in (32, 80], no condition, no
 * output projection, dilations <= 8, DMEL_PRECISION_FP32): everything else is DMEL_EUNSUPPORTED from this entry -- the layered per-item
 * step is dmel_wavenet_stream_step_items_layered below.
 *   scratch: that of dmel_wavenet_stream_step_ex (N * 2 C * cap floats followed by N int64) FOLLOWED BY
 *     (N / group_repeat) * (2 (L + 1) + 1) int32: the rows of a sub-step as the kernel reads them.
 * The host tables are copied as launch arguments: the caller may overwrite them as soon as the call returns.  Every item has the bits
 * dmel_wavenet_stream_step_ex gives it when it is stepped alone (same kernel body, same K order, same epilogues). */
int dmel_wavenet_stream_step_items(const dmel_wavenet* m, const float* x /*nullable*/, float* hist, float* skip, const float* cond /*NULL*/,
                                   float* y, float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                   const int64_t* out_lengths /*nullable*/, int group_repeat, const int64_t* origin, void* stream);

/* The same per-utterance step through the LAYERED path, for every stack dmel_wavenet_stream_step / _ex serve layer by layer: conditioned
 * (cond (N, Ccond, cap), the caller writes its new columns), any width, with or without input and output projection -- the decoder
 * WaveNet of independent live decode sessions.  Arguments, host tables, row checks (a bad row is DMEL_EINVAL naming the utterance, nothing
 * is launched), idle rows and the scratch (table included) are those of dmel_wavenet_stream_step_items.  The rows go to the device once
 * per call, as launch arguments; each of the ~2 L + 3 launches (input projection, L x (gate conv, copy, res / skip conv), skip and
 * output projection) runs over all N items and reads its level's window of every item from that table, so an item's columns have the
 * bits dmel_wavenet_stream_step gives them when that item is stepped alone (same K order, partial products and epilogues; every tile
 * accumulates K in the same order).  The windows are built into the split kernels: DMEL_PRECISION_FP32 / FP32_BF16X3 / FP32_F16X2.  A
 * handle at DMEL_PRECISION_BF16 or FP32_MFMA, or a process with DMEL_CONV_FP32_MFMA set, is DMEL_EUNSUPPORTED with nothing touched. */
int dmel_wavenet_stream_step_items_layered(const dmel_wavenet* m, const float* x /*nullable*/, float* hist, float* skip,
                                           const float* cond /*nullable*/, float* y, float* scratch, int N, int64_t cap, const int64_t* prev,
                                           const int64_t* next, const int64_t* out_lengths /*nullable*/, int group_repeat,
                                           const int64_t* origin, void* stream);

/* Fork the streaming state of some items into other items of the SAME buffers, in one launch: for every row r of the host tables the
 * columns [lo[r], hi[r]) of all channels of item src[r] are copied to item dst[r] -- in every level of hist (L + 1, N, C, cap), in
 * skip (N, C, cap) (its partial sums behind prev[1] are state), in cond (N, Ccond, cap; NULL exactly when Ccond == 0) and in
 * mel (N, Cout, cap), the y of the step.  A decode session that emits early (models/stream_sessions.py: DecodeSessions) steps such a
 * copy to the end of what it has received while the item it was copied from keeps the exact frontiers.  Nothing outside the windows of
 * the dst items is written.  A row with lo == hi is idle.  DMEL_EINVAL, nothing launched, dmel_last_error naming the row: src == dst, a
 * dst that is another row's src or dst, a window outside [0, cap], an item outside [0, N).  src, dst, lo, hi are HOST tables of R rows,
 * copied as launch arguments into table_scratch (5 R int32 of device memory, 4-byte aligned): the caller may overwrite them as soon as
 * the call returns.  The grid covers the columns of the rows' windows, not cap; a (row, channel) whose two addresses are 16-byte
 * aligned and whose lo and hi are multiples of 4 moves 16 bytes per lane, every other one 4. */
int dmel_stream_fork_items(float* hist, float* skip, float* cond /*nullable*/, float* mel, int L, int N, int C, int Ccond, int Cout,
                           int64_t cap, int R, const int64_t* src, const int64_t* dst, const int64_t* lo, const int64_t* hi,
                           void* table_scratch, void* stream);

/* Cross-fade of provisional audio pieces, R rows in ONE launch (csrc/small_ops.hip).  A decode session that emits early hands out
 * pieces cut from different prefix decodes; with a cross-fade of F samples it holds back the last F samples of a piece (the tail) and
 * blends them with the next decode's version of the same samples.  Row r, for i in [0, F[r]):
 *     old = tail[r][i];   if blend[r]: blend[r][i] = old + w[r][i] * (blend[r][i] - old);   if save[r]: tail[r][i] = save[r][i]
 * the blend as three separately rounded fp32 operations (subtract, multiply, add; no fma), bit for bit `old + w * (new - old)` on CPU
 * fp32 torch tensors.  blend[r] (nullable) points at F floats inside the vocoder's output, overwritten in place; save[r] (nullable:
 * the step ends the session) at the F floats that become the new tail; tail[r] and w[r] at F floats of state and F weights.  The
 * blend and save regions of a row MUST NOT overlap and no two rows may share a tail or a region that is written: in a session they
 * are the last F samples in front of, and the last F samples of, a piece of at least one mel frame (`up` >= F samples), which are
 * disjoint.  DMEL_EINVAL, nothing launched, dmel_last_error naming the row: R outside [1, 65535], F[r] outside [1, 4096], a NULL
 * tail or w, a row with neither blend nor save, a pointer that is not 4-byte aligned.  blend, tail, save, w, F are HOST tables of R
 * entries, copied as launch arguments into table_scratch (5 R int64 of device memory, 8-byte aligned): the caller may overwrite them as
 * soon as the call returns.  The grid covers the rows' elements; a row whose F is a multiple of 4 and whose pointers are all 16-byte
 * aligned moves 16 bytes per lane, every other one 4.  No LDS, no atomics. */
int dmel_crossfade_items(float* const* blend /*entries nullable*/, float* const* tail, const float* const* save /*entries nullable*/,
                         const float* const* w, const int64_t* F, int R, void* table_scratch, void* stream);

/* Voice activity and end of turn on log-mel frames, S session slots in ONE launch (csrc/small_ops.hip): the detector of encode
 * sessions opened with voice= (models/stream_sessions.py), whose rule is utils/voice.py -- the kernel equals voice.scan bit for bit.
 * Slot s reads frames t in [0, n_frames[s]) of its bands b in [0, n_mels) at mel[s * item_stride + b * band_stride + t] (strides in
 * floats, frames contiguous) and carries one row of n_mels + 8 4-byte words in `state`: floor[b] (fp32) per band, then eight int32
 * (state: 0 silence / 1 speech, run, seen, start, end, starts, active_frames, one reserved word kept at 0).  A zeroed row is a
 * fresh session: seen == 0 makes the first frame initialise the floors and start = end = -1.  Per frame f = seen, L[b] its column:
 *     fl = seen == 0 ? L[b] : floor[b] + c * (L[b] - floor[b]),  c = L[b] < floor[b] ? fall : state == 0 ? rise : rise_speech
 *          (subtract, multiply, add: three separately rounded fp32 operations, no fma);   floor[b] = fl < min_level ? min_level : fl
 *     count = #{b in [band_lo, band_hi): L[b] > min_level && L[b] - floor[b] > threshold};   active = count >= min_bands
 *     run = (active != (state == 1)) ? run + 1 : 0
 *     state 0 and run >= attack_frames:  state = 1, start = f - run + 1, starts += 1, run = 0
 *     state 1 and run >= release_frames: state = 0, end = f - run + 1, run = 0
 *     seen += 1;  active_frames += active;  flags[s * out_pitch + t] = active | state << 1;  counts[s * out_pitch + t] = count
 * fparams row s is (threshold, min_level, fall, rise, rise_speech), iparams row s (band_lo, band_hi, min_bands, attack_frames,
 * release_frames).  flags and counts (each nullable) are rows of out_pitch bytes; the bytes behind a row's n_frames[s] are not
 * written.  n_frames[s] == 0 is an idle slot: neither its state row nor its output rows nor its parameters are looked at; when
 * every slot is idle the call returns DMEL_OK and launches nothing.  The frame counter is an int32: 2^31 frames, 265 days at 93.75
 * frames per second, which nothing checks.  NaN input is outside the contract.  DMEL_EINVAL, nothing launched, dmel_last_error
 * naming the item: S outside [1, 65535], n_mels outside [1, 128], a NULL mel, state or table, a mel or state pointer that is not
 * 4-byte aligned, negative strides, a negative n_frames[s] or one above 2^31 - 1, out_pitch below a row's frames, a value of fparams
 * that is not finite, threshold <= 0, fall or rise outside (0, 1], rise_speech outside [0, 1], a band window that is not
 * 0 <= lo < hi <= n_mels, min_bands outside [1, hi - lo], attack_frames or release_frames outside [1, 2^20].  n_frames, fparams,
 * iparams are HOST tables, copied as launch arguments into table_scratch (12 S 4-byte words of device memory, 4-byte aligned): the
 * caller may overwrite them as soon as the call returns.  One 64-lane wave per slot: a lane owns bands lane and lane + 64 and keeps
 * their floors in registers for the whole launch; the slot's tile passes through LDS in chunks of 64 frames, read from global memory
 * along the frames; the frame loop is sequential (the coefficient of a frame depends on the state after the one before it), the band
 * count two ballots, the state machine uniform over the wave.  Plain vector stores, no atomics. */
int dmel_voice_items(const float* mel, int64_t item_stride, int64_t band_stride, int n_mels, int S, const int64_t* n_frames,
                     const float* fparams /* S x 5 */, const int32_t* iparams /* S x 5 */, void* state /* (S, n_mels + 8) words */,
                     uint8_t* flags /*nullable*/, uint8_t* counts /*nullable*/, int64_t out_pitch, void* table_scratch, void* stream);

/* DTMF (touch-tone) keys on codec-rate samples, S session slots in ONE launch (csrc/small_ops.hip): the detector of encode sessions
 * opened with dtmf= (models/stream_sessions.py), whose rule, defaults and caveats are utils/dtmf.py -- the kernel equals dtmf.scan bit
 * for bit.  Slot s reads its n_new[s] new samples at samples[s * row_stride + first[s] + i] (fp32, any 4-byte offset) and carries one
 * row of 128 4-byte words in `state`: words 0 .. 7 the s1 and 8 .. 15 the s2 of the eight Goertzel filters in the open (partial)
 * block (rows 697, 770, 852, 941 Hz, then columns 1209, 1336, 1477, 1633 Hz), 16 its energy, all fp32; then int32: 17 fill (samples
 * of the open block consumed), 18 blocks, 19 down, 20 candidate, 21 run, 22 miss_run, 23 events; 24 .. 31 reserved, kept at 0;
 * 32 .. 127 the ring of the last 32 events, (key + 1, start_block, end_block or -1) each, event i at ring[i % 32].  A zeroed row is
 * a fresh session.  Blocks are N[s] consecutive samples, counted from the session's first; a partial last block is never decided.
 * Per block and filter k, in sample order from s1 = s2 = 0:   p = c_k * s1, q = p - s2, s0 = x + q, s2 = s1, s1 = s0   (three
 * separately rounded fp32 operations, no fma);   P_k = (s1 * s1 + s2 * s2) - c_k * (s1 * s2), every operation rounded;   the energy
 * e = e + x * x.  With r / c the argmax of the row / column powers (the lowest index on a tie), the block decides key 4 r + c where
 *     E > emin;   P_r > rel * P_j for the other rows, P_c > rel * P_j for the other columns;   P_c <= max_col_over_row * P_r and
 *     P_r <= max_row_over_col * P_c;   (P_r + P_c) > g * E
 * and nothing otherwise.  The state machine, per decided block b = blocks with decision d (key + 1, or 0):
 *     no key down:  d == 0: candidate = run = 0;  d == candidate: run += 1;  else candidate = d, run = 1;
 *                   candidate and run >= hits: down = candidate, miss_run = 0, ring[events % 32] = (down, b - run + 1, -1), events += 1
 *     a key down:   d == down: miss_run = 0;  else miss_run += 1, and at miss_run >= misses the newest event's end_block =
 *                   b - miss_run + 1 and down = candidate = run = miss_run = 0
 *     blocks += 1;  decided[s * out_pitch + j] = d, pressed[s * out_pitch + j] = down for the j-th block the launch completed
 * coef row s is c_0 .. c_7 = fp32(2 cos(2 pi f_k / rate)), computed by the caller; fparams row s (emin, rel, max_col_over_row,
 * max_row_over_col, g); iparams row s (hits, misses).  The bytes behind the blocks a row completed are not written.  n_new[s] == 0
 * is an idle slot: neither its rows nor its parameters are looked at; when every slot is idle the call returns DMEL_OK and launches
 * nothing.  NaN input is outside the contract.  DMEL_EINVAL, nothing launched, dmel_last_error naming the item: S outside
 * [1, 65535], a NULL pointer, samples, state or table not 4-byte aligned, a negative stride or pitch, n_new[s] or first[s] outside
 * [0, 2^30), N[s] outside [32, 4096], out_pitch below ceil(n_new[s] / N[s]) (the blocks the item can complete with N - 1 samples
 * carried), a coefficient outside [-2, 2], a value of fparams that is not finite and positive, hits or misses outside [1, 2^20].
 * first, n_new, N, coef, fparams, iparams are HOST tables, copied as launch arguments into table_scratch (20 S 4-byte words of device
 * memory, 4-byte aligned): the caller may overwrite them as soon as the call returns.  One workgroup of four waves per slot; nine
 * lanes serve a block (eight filters and the energy), a wave seven blocks, a pass 28; the samples pass through LDS in chunks of 64
 * per block.  Plain vector stores, no atomics. */
int dmel_dtmf_items(const float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new, const int32_t* N,
                    const float* coef /* S x 8 */, const float* fparams /* S x 5 */, const int32_t* iparams /* S x 2 */,
                    void* state /* (S, 128) words */, uint8_t* decided, uint8_t* pressed, int64_t out_pitch, void* table_scratch,
                    void* stream);

/* Input level (a causal block AGC with a meter) on codec-rate samples, S session slots in ONE launch (csrc/small_ops.hip): the
 * leveller of encode sessions opened with level= (models/stream_sessions.py), whose rule, defaults and caveats are utils/level.py -- the
 * kernel equals level.scan bit for bit.  Slot s RE-WRITES IN PLACE its n_new[s] new samples at samples[s * row_stride + first[s] + i]
 * (fp32, any 4-byte offset; no other column is written) and carries one row of 16 4-byte words in `state`: fp32 0 env, 1 ga, 2 gb,
 * 3 open_peak, 4 peak_in, 5 peak_out; int32 6 fill (samples of the open block consumed), 7 blocks, 8 locked, 9 held, 10 clamped;
 * 11 .. 15 reserved and not written.  A zeroed row is a fresh session: while locked == 0, ga and gb read as initial_gain whatever the
 * row holds, and a launch with samples writes back what it read.  Blocks are N[s] consecutive samples, counted from the session's
 * first.  Sample x at position i of the open block, whose start gain is ga and end gain gb (five separately rounded fp32 operations,
 * no fma):
 *     d = gb - ga;  u = (float)(i + 1) * rN;  m = d * u;  gi = ga + m;  y = x * gi;
 *     y > ceiling: y = ceiling, clamped += 1;  y < -ceiling: y = -ceiling, clamped += 1;
 *     open_peak = max(open_peak, |x|);  peak_out = max(peak_out, |y|)
 * A completed block, in block order, p = open_peak:
 *     peak_in = max(peak_in, p);
 *     not locked:  p >= gate: env = p, locked = 1
 *     locked:      p < gate and p < env: held += 1;  else k = p >= env ? attack : release, t = p - env, t = k * t, env = env + t
 *     g = locked ? min(max(target / max(env, emin), min_gain), max_gain) : initial_gain      (the IEEE fp32 division)
 *     ga = gb, gb = g, open_peak = 0, fill = 0, blocks += 1;  out_peak[s * out_pitch + j] = p, out_gain[s * out_pitch + j] = g for the
 *     j-th block the launch completed
 * fparams row s is (initial_gain, target, emin, min_gain, max_gain, attack, release, gate, ceiling, rN), fp32 values computed by the
 * caller (emin = target / max_gain, rN = 1 / N[s]).  The words behind the blocks a row completed are not written.  n_new[s] == 0 is
 * an idle slot: neither its rows nor its parameters are looked at; when every slot is idle the call returns DMEL_OK and launches
 * nothing.  NaN input is outside the contract.  DMEL_EINVAL, nothing launched, dmel_last_error naming the item: S outside [1, 65535],
 * a NULL pointer, samples, state, out_peak, out_gain or table not 4-byte aligned, a negative stride or pitch, n_new[s] or first[s]
 * outside [0, 2^30), N[s] outside [32, 4096], out_pitch below ceil(n_new[s] / N[s]) (the blocks the item can complete with N - 1
 * samples carried), a value of fparams that is not finite and positive (the gate alone may be 0), attack, release or rN above 1,
 * initial_gain outside [min_gain, max_gain].  first, n_new, N and fparams are HOST tables, copied as launch arguments into
 * table_scratch (16 S 4-byte words of device memory, 4-byte aligned): the caller may overwrite them as soon as the call returns.  One
 * workgroup of four waves per slot; a pass takes min(64, 4096 / N) blocks through LDS: read (16 bytes per lane on the aligned body of
 * the range, single words at its ends) and raw block peaks, the recursion in block order, then ramp, gain and clamp back to the row.
 * Plain vector stores, no atomics.  One profile record per launch in the family "level" (time and bytes in "small"). */
int dmel_level_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new, const int32_t* N,
                     const float* fparams /* S x 10 */, void* state /* (S, 16) words */, float* out_peak, float* out_gain,
                     int64_t out_pitch, void* table_scratch, void* stream);

/* Noise suppression (a spectral gain over a learnt and tracked noise power) on codec-rate samples, S session slots in ONE launch
 * (csrc/small_ops.hip): the suppressor of encode sessions opened with denoise= (models/stream_sessions.py), whose rule, constants, table
 * and caveats are utils/denoise.py -- the kernel equals denoise.scan bit for bit.  Slot s RE-WRITES IN PLACE its n_new[s] new samples at
 * samples[s * row_stride + first[s] + i] (fp32, any 4-byte offset; no other column is written) with the suppressed signal delayed by
 * N[s] samples, and carries one row of 3092 4-byte words in `state`: int32 0 frames, 1 fill (samples of the open hop), 2 learned; fp32
 * 3 sum of power_in, 4 sum of power_out, 5 the sum of the noise powers; 6 .. 15 kept at 0; then fp32 raw[1024] at 16 (the last whole
 * hop, then the open hop), tail[512] at 1040, hop[512] at 1552 (the finished hop that streams out), Nz[513] at 2064, prev[513] at
 * 2577.  A zeroed row is a fresh session.  N[s] is the frame, a power of two in 64 .. 1024, the hop is N / 2; frame k is computed when
 * its last sample arrives: sine window, radix-2 FFT, the per-bin recursion, inverse FFT, window, overlap-add, every fp32 operation
 * rounded on its own in the order utils/denoise.py states.  power_in[s * out_pitch + j] = the sum of the bin powers of the j-th frame
 * the launch completed, power_out[...] the same behind the gain.  fparams row s is (alpha, 1 - alpha, track, track_ratio, creep,
 * floor_gain, eps, 1 / N), fp32 values computed by the caller; learn_frames[s] in 1 .. 4096.  transform: the constant table of 3072
 * fp32 words on the device (sin(pi k / 2048), k < 2048; cos(2 pi k / 1024), k < 512; sin(2 pi k / 1024), k < 512), computed in float64
 * by the caller and rounded once; no trigonometry runs on the device.  The words behind the frames a row completed are not written.
 * n_new[s] == 0 is an idle slot: neither its rows nor its parameters are looked at; when every slot is idle the call returns DMEL_OK
 * and launches nothing.  NaN input is outside the contract.  DMEL_EINVAL, nothing launched, dmel_last_error naming the item: S outside
 * [1, 65535], a NULL pointer, a pointer not 4-byte aligned, a negative stride or pitch, n_new[s] or first[s] outside [0, 2^30), N[s] no
 * power of two in [64, 1024], out_pitch below ceil(n_new[s] / (N[s] / 2)), learn_frames[s] outside [1, 4096], a value of fparams
 * that is not finite or outside its range (alpha [0, 1), 1 - alpha (0, 1], track (0, 1], track_ratio [1, 1e6], creep [1, 2],
 * floor_gain [1e-6, 1], eps [1e-30, 1]), rN that is not 1 / N[s].  The host tables are copied as launch arguments into table_scratch
 * (16 S 4-byte words of device memory): the caller may overwrite them as soon as the call returns.  One workgroup of four waves per
 * slot, 2 log2 N + 5 barriers per frame; plain stores, no atomics.  One profile record per launch in the family "denoise" (time and
 * bytes in "small"). */
int dmel_denoise_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new, const int32_t* N,
                       const int32_t* learn_frames, const float* fparams /* S x 8 */, void* state /* (S, 3092) words */,
                       float* power_in, float* power_out, int64_t out_pitch, const float* transform /* 3072 words */,
                       void* table_scratch, void* stream);

/* Echo cancellation (a block NLMS adaptive FIR with a meter) on codec-rate samples, S session slots in ONE launch
 * (csrc/small_ops.hip): the canceller of encode sessions opened with echo= (models/stream_sessions.py), whose rule, defaults and caveats
 * are utils/echo.py -- the kernel equals echo.scan bit for bit.  Slot s first appends its far_n[s] new far-end samples far[s][i] (fp32)
 * to the far history in its state row, then RE-WRITES IN PLACE its n_new[s] new samples at samples[s * row_stride + first[s] + i]
 * (fp32, any 4-byte offset; no other column is written) with e = d - yhat.  The state row of slot s is the 68112 4-byte words at
 * state + s * state_pitch words: int32 0 T (samples seen), 1 F (far samples pushed), 2 fill (samples of the open block), 3 blocks,
 * 4 adapted, 5 frozen, 6 far_missing; fp32 7 sd, 8 se; 9 .. 15 reserved and not written; fp32 w[2048] at 16 (the first L are used), the
 * open block's e at 2064 and d at 2320 (256 words each: `fill` values, 0 behind them), and at 2576 a ring of 65536 fp32: far sample
 * x[j] at word j mod 65536.  A zeroed row is a fresh session.  With xd[t] = x[t - delay] (0 where t < delay; 0, counted in far_missing
 * and kept 0, where x[t - delay] had not been appended when sample t was processed -- a far sample appended behind its turn is
 * dropped), sum8 the sum of 8 contiguous segments (boundaries floor(q n / 8)), each ascending from 0.0f, combined as ((s0 + s1) +
 * (s2 + s3)) + ((s4 + s5) + (s6 + s7)), and every product, sum and division a separately rounded fp32 operation (no fma):
 *     sample t:   yhat = sum8_k(w[k] * xd[t - k]), k < L;  e = d - yhat
 *     a completed block of N samples from t0, in block order:
 *       E = sum8(xd[j]^2), mx = max |xd[j]| over j in [t0 - L + 1, t0 + N);  Ed = sum8(d^2), Ee = sum8(e^2), md = max |d| over the block
 *       adapt = E >= far_floor && !(double_talk > 0 && md > double_talk * mx);  !adapt: frozen += 1
 *       adapt: step = mu / (fN * E + eps);  every k: w[k] = w[k] + step * sum8_i(e[i] * xd[t0 + i - k]), i < N;  adapted += 1
 *       sd = sd + meter * (Ed - sd);  se = se + meter * (Ee - se);  blocks += 1
 *       out_in[s * out_pitch + j] = Ed, out_res[s * out_pitch + j] = Ee for the j-th block the launch completed
 * iparams row s is (L, N, delay), fparams row s (mu, eps, far_floor, double_talk, meter, fN = (float)N).  The words behind the blocks a
 * row completed are not written.  n_new[s] == 0 && far_n[s] == 0 is an idle slot: neither its rows nor its parameters are looked at;
 * when every slot is idle the call returns DMEL_OK and launches nothing.  The caller keeps F within 39232 samples ahead of T (what the
 * ring holds next to the longest delay, filter and block): the kernel drops the samples of an append beyond that.  NaN input is
 * outside the contract.  DMEL_EINVAL, nothing launched, dmel_last_error naming the item: S outside [1, 65535], a NULL pointer,
 * samples, state, out_in, out_res or table not 4-byte aligned, a negative stride or pitch, state_pitch below 68112, n_new[s], far_n[s]
 * or first[s] outside [0, 2^30), far[s] NULL or unaligned with far_n[s] > 0, L no multiple of 64 in [64, 2048], N no multiple of 8 in
 * [16, 256], delay outside [0, 24000], out_pitch below ceil(n_new[s] / N) (the blocks the item can complete with N - 1 samples
 * carried), a value of fparams that is not finite and positive (far_floor and double_talk may be 0), mu not below 2, meter above 1,
 * fN != N.  first, n_new, far, far_n, iparams and fparams are HOST tables, copied as launch arguments into table_scratch (16 S 4-byte
 * words of device memory, 4-byte aligned): the caller may overwrite them as soon as the call returns.  One workgroup of four waves per
 * slot; a pass takes 2048 / N blocks through LDS, block by block: the (sample, segment) partial dots, the block's energies and the
 * decision, the tap update; w stays in LDS for the launch.  Plain vector stores, no atomics.  One profile record per launch in the
 * family "echo" (time, flops and bytes in "small"). */
int dmel_echo_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new, const void* const* far,
                    const int64_t* far_n, const int32_t* iparams /* S x 3 */, const float* fparams /* S x 6 */,
                    void* state /* S rows of 68112 words */, int64_t state_pitch, float* out_in, float* out_res, int64_t out_pitch,
                    void* table_scratch, void* stream);

/* Packet-loss concealment (pitch waveform repetition) on codec-rate samples, S session slots in ONE launch (csrc/small_ops.hip): the
 * concealment of encode sessions opened with conceal= (models/stream_sessions.py), whose rule, defaults and caveats are
 * utils/conceal.py -- the kernel equals conceal.scan bit for bit.  Slot s takes its n_new[s] new samples at
 * samples[s * row_stride + first[s] + i] (fp32, any 4-byte offset) through the rule; the n_ranges[s] <= 16 ranges [lo, hi) at
 * ranges[(s * 16 + r) * 2], relative to first[s], are lost: their content is ignored.  Samples are RE-WRITTEN IN PLACE only inside
 * lost ranges and the recovery stretches behind them; no other column is written.  The state row of slot s is the 4112 4-byte words
 * at state + s * state_pitch words: int32 0 T (samples seen), 1 phase (0 good, 1 lost, 2 recovering), 2 t0 (the onset), 3 P (the
 * period, 0: none), 4 k (samples since the onset), 5 rec (recovery samples left), 6 lost, 7 runs, 8 muted, 9 longest, 10 run (length
 * of the open or last run); fp32 11 q (score of the last search), 12 e0 (its window energy); 13 .. 15 reserved and not written; at
 * 16 a ring of 4096 fp32: the slot's OUTPUT sample y[t] at word t mod 4096.  A zeroed row is a fresh session.  With sum8 the sum of
 * 8 contiguous segments, each ascending from 0.0f, combined as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), and every product,
 * sum and division a separately rounded fp32 operation (no fma), per sample in order:
 *     a lost sample with phase != 1, the onset:  t0 = T, k = P = run = 0, q = e0 = 0, runs += 1, phase = 1; if T >= W + Pmax:
 *       a[i] = ring[t0 - W + i], e0 = sum8(a a); if e0 >= floor, over the lags p in [Pmin, Pmax]: b[i] = ring[t0 - W + i - p],
 *       c = sum8(a b), e = sum8(b b), q(p) = c > 0 ? (c c) / (e + eps) : 0; q = the largest q(p), P its lowest lag, P = 0 if q == 0;
 *       out_period[s * out_pitch + j] = P, out_score[s * out_pitch + j] = q for the j-th onset of the launch
 *     s(k) = 0 if P == 0 or k >= H + D; else v = ring[t0 - P + k mod P]; k < H: s = v; else u = (float)(k - H) rD, g = 1.0f - u, s = g v
 *     a lost sample:  y = s(k), k += 1, lost += 1, run += 1, muted += 1 where s(k) was the 0 of the first case
 *     a good sample with phase == 1:  longest = max(longest, run), phase = 2, rec = F
 *     a good sample with rec > 0:  w = (float)(F - rec + 1) rF, d = x - s(k), m = w d, y = s(k) + m, k += 1, rec -= 1, phase = 0 at rec == 0
 *     any other good sample:  y = x;       always:  ring[T mod 4096] = y, T += 1
 * iparams row s is (W, Pmin, Pmax, H, D, F), fparams row s (floor, eps, rD = fp32(1 / D), rF = fp32(1 / (F + 1))).  The words of
 * out_period and out_score behind the onsets a row had are not written.  n_new[s] == 0 is an idle slot: neither its rows nor its
 * parameters are looked at; when every slot is idle the call returns DMEL_OK and launches nothing.  NaN input is outside the contract.
 * DMEL_EINVAL, nothing launched, dmel_last_error naming the item: S outside [1, 65535], a NULL pointer, samples, state, out_period,
 * out_score or table not 4-byte aligned, a negative stride or pitch, state_pitch below 4112, n_new[s] or first[s] outside [0, 2^30),
 * n_ranges[s] outside [0, 16], a range that is empty, outside [0, n_new[s]], or not behind the one in front of it with a gap (ranges
 * are sorted and do not touch), W no multiple of 8 or below 8, Pmin < 8, Pmin > Pmax, W + Pmax > 4096, H < 0, D < 0,
 * H + D + Pmax > 4096, F < 1, out_pitch below n_ranges[s], floor or rD not finite or negative, eps or rF not finite and positive, rF
 * above 1.  first, n_new, n_ranges, ranges, iparams and fparams are HOST tables, copied as launch arguments into table_scratch (48 S
 * 4-byte words of device memory, 4-byte aligned): the caller may overwrite them as soon as the call returns.  One workgroup of four
 * waves per slot, the ring in LDS for the launch; the row's good and lost stretches are walked in order, each of them in parallel: a
 * good stretch is a copy into the ring, an onset the (lag, segment) partial sums over the lanes, the fixed tree and a workgroup
 * argmax on (q, -lag), a lost run and a recovery one lane per sample.  Plain vector stores, no atomics.  One profile record per
 * launch in the family "conceal" (time and bytes in "small"). */
int dmel_conceal_items(float* samples, int64_t row_stride, int S, const int64_t* first, const int64_t* n_new,
                       const int32_t* n_ranges /* S */, const int32_t* ranges /* S x 16 x 2, relative to first[s] */,
                       const int32_t* iparams /* S x 6: W, Pmin, Pmax, H, D, F */, const float* fparams /* S x 4: floor, eps, rD, rF */,
                       void* state /* S rows */, int64_t state_pitch, int32_t* out_period, float* out_score, int64_t out_pitch,
                       void* table_scratch, void* stream);

/* Tones spliced into codec-rate audio, R parts in ONE launch (csrc/small_ops.hip): what decode sessions of a pool built with
 * tones=True send DTMF keys, beeps and call-progress tones with (models/stream_sessions.py: send_dtmf / send_tones), whose rule, tables
 * and caveats are utils/tones.py -- the kernel equals tones.render bit for bit.  Part r writes n[r] floats at dst[r].  Where src[r] is
 * not NULL the part is a copy of n[r] floats from src[r] (words move as uint32: nothing is canonicalised).  Otherwise it is the
 * rendering of the segments [seg_first[r], seg_first[r] + seg_count[r]), 1 .. 64 of them, of the launch's segment table `segs`, and
 * n[r] must equal their total length.  Tone parts may name the same segments only where every shared segment begins at the same
 * sample of both parts (equal ranges, or ranges with one first segment): the table holds one prefix sum per segment, and a segment
 * that a second part would begin elsewhere is refused.  A spliced piece is three or more parts with consecutive dst: head, tone,
 * tail.  A segment is eight 4-byte words: f1, f2 (int32 Hz, 0 <= f < rate / 2; f = 0 goes with a = 0: no such tone), a1, a2 (fp32, finite, >= 0,
 * a1 + a2 <= 1), on, off, ramp (int32 samples, 1 <= on < 2^24, 0 <= off < 2^24, 0 <= ramp <= min(on / 2, 4096)) and ramp_off, the
 * offset of the segment's ramp table in `ramps` (not looked at where ramp == 0).  `sine` holds `rate` floats, sine[j] =
 * fp32(sin(2 pi j / rate)); the ramp table of a segment holds `ramp` floats, RAMP[i] = fp32(0.5 - 0.5 cos(pi (i + 0.5) / ramp)); both
 * are computed by the caller in float64 and rounded once: the kernel evaluates no sine and no cosine.  Sample i of a segment,
 * 0 <= i < on:
 *     p_k = (f_k * i) mod rate (exact, 64-bit; the phase starts at 0 in every segment);   t_k = a_k * sine[p_k];   x = t_1 + t_2;
 *     g = RAMP[i] for i < ramp, RAMP[on - 1 - i] for i >= on - ramp, 1.0f otherwise;   y = x * g
 * four separately rounded fp32 operations, no fma; the samples on .. on + off - 1 are +0.0f.  n[r] == 0 is an idle part: neither its
 * pointers nor its segments are looked at; when every part is idle the call returns DMEL_OK and launches nothing.  DMEL_EINVAL,
 * nothing launched, dmel_last_error naming the part: R outside [1, 65535], a NULL table, sine or table_scratch, a NULL segs with
 * n_segs > 0 or ramps with ramp_floats > 0, n_segs outside [0, 64 * 65535], rate outside [4000, 192000], a sine, ramps, dst or src
 * that is not 4-byte aligned, a table_scratch that is not 8-byte aligned, n[r] negative or 2^40 and more, a NULL dst of a live part,
 * a segment range outside the table or of no or more than 64 segments, a segment field outside the bounds above, ramp_off + ramp
 * beyond ramp_floats, a part whose length is not the total length of its segments, a segment that begins at another sample of
 * this part than of an earlier part that names it.  OVERLAP IS THE CALLER'S CONTRACT, as in
 * dmel_stream_pack_items below: nothing checks that a destination is not another part's destination or source.  dst, src, n,
 * seg_first, seg_count and segs are HOST tables, copied as launch arguments into table_scratch (6 R + 5 n_segs int64 of device
 * memory, 8-byte aligned): the caller may overwrite them as soon as the call returns.  The grid covers the parts' own tiles of 1024
 * floats, four per lane, laid on the 16-byte grid of each destination: every lane stores 16 bytes but the two that meet the ends of a
 * part, which store single floats; both store paths give the same bits.  A lane finds its segment from the part's prefix sums.  Plain
 * vector stores, no LDS, no atomics.  One profile record per launch in the family "tones" (time and bytes in "small"). */
int dmel_tone_items(float* const* dst, const float* const* src /*entries nullable*/, const int64_t* n, const int32_t* seg_first,
                    const int32_t* seg_count, int R, const int32_t* segs /* n_segs x 8 words, nullable when n_segs == 0 */, int n_segs,
                    const float* sine /* rate floats */, int rate, const float* ramps /*nullable when ramp_floats == 0*/,
                    int64_t ramp_floats, void* table_scratch, void* stream);

/* Reply shaping on codec-rate audio, S session slots in ONE launch (csrc/small_ops.hip): a commanded gain that ramps between requests,
 * a block look-ahead limiter and a flush at the end of the stream, for decode sessions opened with shape= (models/stream_sessions.py),
 * whose rule, defaults and caveats are utils/shape.py -- the kernel equals shape.scan bit for bit.  Slot s takes n_new[s] new floats z
 * at src[s] (any 4-byte offset) and writes the samples that leave to dst[s] (ANOTHER buffer than src[s]: the counts differ; any 4-byte
 * offset).  flags[s]: bit 0 final (the session's last step: everything held leaves), bit 1 limit.  It carries one row of state_pitch
 * 4-byte words in `state`: a header of 16 words -- fp32 0 s, 1 node, 2 open_peak; int32 3 hold, 4 blocks, 5 in, 6 out; fp32 7 c_now,
 * 8 s_min; int32 9 limited, 10 clamped; fp32 11 peak_in, 12 peak_out; 13 .. 15 reserved and not written -- and, with the limiter,
 * 2 N[s] - 1 floats: the held samples of v, oldest first, zeros behind them.  A zeroed row is a fresh session: while in == 0, s, node
 * and s_min read as 1.0f whatever the row holds.
 *   Commanded gain of new sample i (0-based in this launch): the last of the slot's seg_count[s] <= 8 segment records -- five 4-byte
 * words at segs[(8 s + k) * 5]: start (int32, relative to the launch's first new sample, may be negative, non-decreasing in k), ramp
 * (int32, 0 .. 16384), ramp_off (int32, offset of its table in `ramps`, not looked at where ramp == 0), g0, g1 (fp32 in
 * [0, max_gain]) -- with start <= i; none: c = base.  at = i - start:  at < ramp: d = g1 - g0, m = d * ramps[ramp_off + at],
 * c = g0 + m (separately rounded, no fma);  else c = g1.  A ramp table holds RAMP[k] = fp32(0.5 - 0.5 cos(pi (k + 0.5) / ramp)),
 * computed by the caller in float64.  v = z * c.
 *   Limiter: the local stream is the hold[s] held samples followed by the new v; blocks are N[s] samples.  hold[s] is the HOST's count
 * of the samples the row holds (the caller tracks it from the rule's integers; the kernel trusts it and writes it back), 0 .. 2 N - 1;
 * at hold >= N the first block is the whole one an earlier launch completed and its start node is word 1.  A completed block b, in
 * block order, p = max |v| over it:
 *     t = p > ceiling ? ceiling / p : 1.0f (IEEE division);  u = 1.0f - s;  u = release * u;  r = s + u;  s_b = min(t, r);
 *     n_b = min(s, s_b);  s = s_b;  s_min = min(s_min, s_b);  limited += p > ceiling;  blocks += 1;
 *     out_peak[s * out_pitch + j] = p, out_gain[s * out_pitch + j] = s_b for the j-th block the launch completed
 * Block b leaves when block b + 1 is complete; sample i of it:
 *     d = n_{b+1} - n_b;  u = (float)(i + 1) * rN;  m = d * u;  gi = n_b + m;  y = v * gi;
 *     y > ceiling: y = ceiling, clamped += 1;  y < -ceiling: y = -ceiling, clamped += 1;  peak_out = max(peak_out, |y|)
 * so a launch that is not final hands out max(0, (hold + n_new) / N - 1) * N samples.  A final launch completes the open block over the
 * samples it has, sets the node behind the last block to s, and hands out hold + n_new samples.  Without the limiter y = clamp(v),
 * n_new samples leave and hold[s] must be 0.  fparams row s is (ceiling, release, rN, base, max_gain), fp32 values computed by the
 * caller.  n_new[s] == 0 without final is an idle slot: neither its rows nor its parameters are looked at; when every slot is idle
 * the call returns DMEL_OK and launches nothing.  NaN and infinite input are outside the contract.  DMEL_EINVAL, nothing launched,
 * dmel_last_error naming the item: S outside [1, 65535], a NULL table, a NULL ramps with ramp_floats > 0, state, out_peak, out_gain
 * or ramps not 4-byte aligned, table_scratch not 8-byte aligned, state_pitch below 16 or a negative out_pitch, n_new[s] outside
 * [0, 2^30), flags[s] outside [0, 3], N[s] outside [32, 1024] with the limiter, hold[s] outside [0, 2 N - 1] (not 0 without the
 * limiter), state_pitch below 16 + 2 N - 1, out_pitch below the blocks the step completes, dst_cap[s] BELOW THE SAMPLES THE STEP
 * HANDS OUT, a NULL dst where samples leave or src where n_new > 0, a dst or src that is not 4-byte aligned, a value of fparams that is
 * not finite and positive (the base gain alone may be 0), release or rN above 1, base above max_gain, more than 8 segments, a start
 * outside [-2^30, 2^30] or below the one before, a ramp outside [0, 16384] or a table beyond ramp_floats, a g0 or g1 that is not
 * finite in [0, max_gain].  OVERLAP IS THE CALLER'S CONTRACT, as in dmel_tone_items.  The per-slot arguments are HOST tables, copied
 * as launch arguments into table_scratch (64 S 4-byte words of device memory, 8-byte aligned): the caller may overwrite them as soon
 * as the call returns.  One workgroup of four waves per slot; a pass takes min(63, 4096 / N) + 1 blocks through LDS and emits all
 * but the last: gain and block peaks (wave reductions), the recursion on one lane, then ramp, gain, clamp and the store; the new
 * hold goes back to the row behind the last pass.  Plain vector stores, no atomics.  One profile record per launch in the family
 * "shape" (time and bytes in "small"). */
int dmel_shape_items(float* const* dst /*entries nullable*/, const int64_t* dst_cap, const float* const* src /*entries nullable*/,
                     const int64_t* n_new, const int64_t* hold, const int32_t* flags, const int32_t* N,
                     const float* fparams /* S x 5 */, const int32_t* seg_count, const int32_t* segs /* S x 8 x 5 words */, int S,
                     const float* ramps /*nullable when ramp_floats == 0*/, int64_t ramp_floats, void* state /* (S, state_pitch) words */,
                     int64_t state_pitch, float* out_peak, float* out_gain, int64_t out_pitch, void* table_scratch, void* stream);

/* The speaking rate of S decode sessions in ONE launch (csrc/small_ops.hip): WSOLA time-scaling of codec-rate speech, the rule of
 * dmel_codec_amd/utils/pace.py (scan), bit for bit; fp32 throughout, every operation rounded on its own, IEEE divisions, every sum
 * in the sum8 order of dmel_echo_items.  Slot s takes n_new[s] new fp32 samples at src[s] (any 4-byte offset) as x[fed ...] and writes
 * the samples the step hands out to dst[s] (ANOTHER buffer than src[s]: the counts differ; any 4-byte offset).  flags[s]: bit 0 final
 * (the stream's last step).  It carries one row of state_pitch 4-byte words in `state`: a header of 16 words -- int32 0 K, 1 p_{K-1},
 * 2 a_{K-1}, 3 a_K, 4 fed, 5 hold, 6 natural, 7 searched, 8 quiet, 9 out, 10 last offset; fp32 11 last q; int32 12 the rate that placed
 * a_K; 13 .. 15 reserved and not written -- and 2 H + 2 D floats: the held samples x[fed - hold, fed), oldest first, zeros behind them.
 * A zeroed row is a fresh session.  ints row s is (K, a_{K-1}, a_K, fed, hold), the HOST's integers (the caller tracks them from the
 * rule's integer helpers; the kernel trusts them and writes them back); p_{K-1} and the counters are the row's.
 *   Frames: output frame k has the nominal position a_k, a_0 = 0, a_{k+1} = a_k + (H r + 500) / 1000 with r the rate in force at input
 * position a_k: that of the last of the slot's req_count[s] <= 8 request records -- two int32 at reqs[(8 s + j) * 2]: position relative
 * to the launch's first new sample (may be negative, non-decreasing in j) and permille -- with position <= a_k - fed, else
 * base_permille[s].  A step that is not final computes frame 0 when fed + n_new >= H and frame k >= 1 when fed + n_new >=
 * max(a_{k-1} + 2 H, a_k + H) + D; a final step computes every frame with a_k < fed + n_new, and its last frame hands out
 * min(H, fed + n_new - a_k) samples; every other frame hands out H.  Samples at or behind fed + n_new read as 0.0.
 *   Frame 0 is x[0 : H].  Frame k >= 1, t = p_{k-1} + H, old[i] = x[t + i]:  a_k - D <= t <= a_k + D: p_k = t (natural += 1);  else
 * e0 = sum8(old * old) < floor: p_k = a_k (quiet += 1);  else for every d in [-D, D] with c = a_k + d >= 0, b[i] = x[c + i]:
 * cc = sum8(old * b), e = sum8(b * b), q = cc > 0 ? (cc * cc) / (e + eps) : 0, and p_k = a_k + d for the d with the largest q, among
 * equal values the smallest |d|, then the negative one (searched += 1).  Sample i of the frame: p_k == t: old;  else m = x[p_k + i] -
 * old, m = W[i] * m, y = old + m, W the H floats at weights + weight_off[s]: W[i] = fp32(0.5 - 0.5 cos(pi (i + 0.5) / H)), computed by
 * the caller in float64.  out_offset[s * out_pitch + j] = p - a and out_score[s * out_pitch + j] = q (0 unless searched) for the j-th
 * frame the launch completed.  Behind the step the row holds x[keep, fed + n_new), keep = max(0, min(a_{K-1} + H, a_K) - D) (0 while
 * K == 0); a final step keeps nothing.  fparams row s is (floor, eps).  n_new[s] == 0 without final is an idle slot: neither its rows
 * nor its parameters are looked at; when every slot is idle the call returns DMEL_OK and launches nothing.  NaN and infinite input
 * are outside the contract.  DMEL_EINVAL, nothing launched, dmel_last_error naming the item: S outside [1, 65535], a NULL table, a
 * negative weight_floats, state, out_offset, out_score or weights not 4-byte aligned, table_scratch not 8-byte aligned, state_pitch
 * below 16 or a negative out_pitch, n_new[s] outside [0, 2^26], flags[s] outside [0, 1], H[s] outside [64, 512] or no multiple of 8,
 * D[s] outside [0, 512], hold AT OR ABOVE 2 H + 2 D, state_pitch below 16 + 2 H + 2 D, fed below hold or above 2^30, integers the rule
 * cannot have made (K < 0; K == 0 with a_K != 0; a_K - a_{K-1} outside [H / 2, 2 H]; a_K above fed + 2 H), a dst or src that is not
 * 4-byte aligned, a floor that is not finite and >= 0 or an eps that is not finite and positive, a base rate or a request's rate
 * outside [500, 2000], more than 8 requests, a request position outside [-2^30, 2^30] or below the one before, a weight table beyond
 * weight_floats, out_pitch below the frames the step completes, dst_cap[s] BELOW THE SAMPLES THE STEP HANDS OUT, a NULL dst where
 * samples leave or src where n_new > 0.  OVERLAP IS THE CALLER'S CONTRACT, as in dmel_tone_items.  The per-slot arguments are HOST
 * tables, copied as launch arguments into table_scratch (64 S 4-byte words of device memory, 8-byte aligned): the caller may
 * overwrite them as soon as the call returns.  One workgroup of eight waves per slot, its frames in order; a window of 6144 samples
 * of the slot's stream sits in LDS and is re-filled as the frames advance; in a searched frame the work items are (candidate, sum8
 * segment) pairs spread over the workgroup, joined per candidate by the fixed tree, and the argmax is a reduction over (q, |d|, d)
 * keys.  Plain vector stores, no atomics.  One profile record per launch in the family "pace" (time and bytes in "small"). */
int dmel_pace_items(float* const* dst /*entries nullable*/, const int64_t* dst_cap, const float* const* src /*entries nullable*/,
                    const int64_t* n_new, const int64_t* ints /* S x 5 */, const int32_t* flags, const int32_t* H, const int32_t* D,
                    const float* fparams /* S x 2 */, const int32_t* base_permille, const int32_t* req_count,
                    const int32_t* reqs /* S x 8 x 2 words */, int S, const float* weights, int64_t weight_floats,
                    const int32_t* weight_off, void* state /* (S, state_pitch) words */, int64_t state_pitch, int32_t* out_offset,
                    float* out_score, int64_t out_pitch, void* table_scratch, void* stream);

/* R independent 2-D copies of 4-byte words in ONE launch (csrc/small_ops.hip): what takes the streaming state of live sessions out of
 * a pool's buffers into a snapshot and back (models/stream_sessions.py: snapshot / restore).  Descriptor r copies rows[r] rows of
 * cols[r] words: row i goes from src[r] + i * src_pitch[r] to dst[r] + i * dst_pitch[r], pitches in words.  Packing reads windows of
 * rows of pitch `cap` and writes a dense blob (pitch == cols); unpacking is the same call with the roles swapped, into rows of any
 * other pitch.  Words move as uint32: NaN payloads and int32 ids come out bit for bit, nothing is canonicalised, no float arithmetic
 * is done.  A descriptor with rows * cols == 0 is idle and its pointers and pitches are not looked at; when every descriptor is idle
 * the call returns DMEL_OK and launches nothing.  DMEL_EINVAL, nothing launched, dmel_last_error naming the row: R outside
 * [1, 65535], a negative count, a NULL or not 4-byte aligned pointer on either side of a live row, a pitch below cols where
 * rows > 1 (the pitches of a single row are ignored), rows * pitch (or rows, or cols) of 2^40 or more, more than 2^31 - 1 tiles.
 * OVERLAP IS THE CALLER'S CONTRACT: nothing checks that the destination of one descriptor is not the source or the destination of
 * another (or of itself); the result of such a call is undefined.  src, dst, rows, cols, src_pitch, dst_pitch are HOST tables of R
 * entries, copied as launch arguments into table_scratch (8 R int64 of device memory, 8-byte aligned): the caller may overwrite them
 * as soon as the call returns.  The grid covers the descriptors' own tiles of 8 rows x 256 words, not a bounding box.  A descriptor
 * whose two base addresses are 16-byte aligned and, where rows > 1, whose two pitches are multiples of 4 words moves 16 bytes per
 * lane and the last cols % 4 words of a row one by one; every other descriptor moves 4 bytes per lane.  Both paths give the same
 * bits.  No LDS, no atomics. */
int dmel_stream_pack_items(const void* const* src, void* const* dst, const int64_t* rows, const int64_t* cols, const int64_t* src_pitch,
                           const int64_t* dst_pitch, int R, void* table_scratch, void* stream);

/* ConvNeXtBlock (models/modules/firefly.py:337-402; C-ABI row `convnext_block`), standalone: y = x + gamma * pwconv2(gelu(pwconv1(
 * LayerNorm_C(dwconv7(x))))), x / y (N, dim, T).  set_tensor keys: dwconv.weight (dim,1,7), dwconv.bias, norm.weight, norm.bias,
 * pwconv1.weight (4 dim, dim), pwconv1.bias, pwconv2.weight (dim, 4 dim), pwconv2.bias, gamma.  The training entry points follow the
 * WaveNet ones (enable_training before finalize; forward_train keeps its intermediates in the workspace that backward is given again;
 * parameter gradients in one flat buffer addressed through grad_slot; dx is always produced).  dim <= 494 (one [dim][33] fp32 tile in
 * the 64 KiB LDS; forward returns an error above it and writes nothing); a TRAINING handle has dim <= 246 (the LayerNorm backward keeps
 * two such tiles): finalize refuses a larger one with DMEL_EUNSUPPORTED, and so does dmel_quantizer_finalize for dim_per_group. */
typedef struct dmel_convnext dmel_convnext;
int dmel_convnext_create(dmel_convnext** m, int dim);
void dmel_convnext_destroy(dmel_convnext* m);
int dmel_convnext_set_tensor(dmel_convnext* m, const char* key, const float* data_host, const int64_t* shape, int ndim);
int dmel_convnext_enable_training(dmel_convnext* m, int on);
int dmel_convnext_set_train_precision(dmel_convnext* h, int precision);   /* see dmel_wavenet_set_train_precision */
int dmel_convnext_finalize(dmel_convnext* m);
size_t dmel_convnext_workspace_bytes(const dmel_convnext* m, int N, int64_t T);
int dmel_convnext_forward(const dmel_convnext* m, const float* x, float* y, int N, int64_t T, void* workspace, size_t workspace_bytes,
                          void* stream);
/* The block over rows of DIFFERENT lengths: lengths_dev (N) device int64; y[n, :, :lengths[n]] is BIT-IDENTICAL to dmel_convnext_forward on
 * x[n:n+1, :, :lengths[n]] and the rest of the row is 0.  The depthwise convolution never reads x at or behind a row's length. */
int dmel_convnext_forward_items(const dmel_convnext* m, const float* x, const int64_t* lengths_dev, float* y, int N, int64_t T,
                                void* workspace, size_t workspace_bytes, void* stream);
size_t dmel_convnext_train_workspace_bytes(const dmel_convnext* m, int N, int64_t T);
int64_t dmel_convnext_grad_floats(const dmel_convnext* m);
int dmel_convnext_grad_slot(const dmel_convnext* m, const char* key, int64_t* offset, int64_t* numel);
int dmel_convnext_forward_train(const dmel_convnext* m, const float* x, float* y, int N, int64_t T, void* workspace,
                                size_t workspace_bytes, void* stream);
int dmel_convnext_backward(const dmel_convnext* m, const float* x, const float* dy, float* dx, float* grads, int N, int64_t T,
                           void* workspace, size_t workspace_bytes, void* stream);

/* DownsampleFiniteScalarQuantize (is_dmel=True, n_codebooks=1)   replaces models/modules/dowmsample_fsq.py:124-147
 * and vector_quantize_pytorch GroupedResidualFSQ.forward / get_output_from_indices. */
typedef struct dmel_quantizer dmel_quantizer;
int dmel_quantizer_create(dmel_quantizer** q, int input_dim /*= groups * dim_per_group*/, int n_groups,
                          const int* levels, int n_levels, const int* downsample_factor, int n_factors,
                          int fsq_prebound);
void dmel_quantizer_destroy(dmel_quantizer* q);
/* Strict encode ("hard parts"): project_in (Linear C -> n_levels) and the tanh bound(s) of
 * dmel_quantizer_encode are evaluated in float64 and rounded to fp32 once, so the value that is rounded to an id no longer depends
 * on a summation order or a tanhf implementation.  Off by default (the fp32 path follows the reference's arithmetic). */
int dmel_quantizer_set_strict(dmel_quantizer* q, int on);
int dmel_quantizer_set_tensor(dmel_quantizer* q, const char* key, const float* data_host, const int64_t* shape, int ndim);
int dmel_quantizer_finalize(dmel_quantizer* q);
size_t dmel_quantizer_workspace_bytes(const dmel_quantizer* q, int B, int64_t T);
/* z (B*G, C, T) -> ids (B, G, T4) int32, T4 = T / prod(factors).  prequant (optional, may be NULL):
 * (G, B, T4, n_levels) fp32, the bounded value that is rounded (for the near-tie analysis of the tests). */
int dmel_quantizer_encode(const dmel_quantizer* q, const float* z, int32_t* ids, float* prequant, int B, int64_t T,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The same, additionally returning the down-sampled features the FSQ sees -- latents (B*G, C, T4), nullable -- so that a checker can
 * feed another FSQ implementation exactly the same input (strict-mode parity test). */
int dmel_quantizer_encode_ex(const dmel_quantizer* q, const float* z, int32_t* ids, float* prequant /*nullable*/,
                             float* latents /*nullable*/, int B, int64_t T, void* workspace, size_t workspace_bytes, void* stream);
/* ids (B, G, T4) -> z (B, G*C, T4*prod(factors)) */
int dmel_quantizer_decode(const dmel_quantizer* q, const int32_t* ids, float* z, int B, int64_t T4,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Both directions over items of DIFFERENT lengths (extension: a pool of live sessions whose windows differ quantises all of them at
 * once).  z (B*G, C, T) / ids (B, G, T4) hold the items right-padded to the largest; lengths_dev (B) is a device int64 array, in feature
 * frames for encode and in tokens for decode, clamped into [0, T] / [0, T4] on the device (never read by the host, no synchronisation).
 *   encode_items: ids[b, :, :lengths[b] / 4] is BIT-IDENTICAL to dmel_quantizer_encode on z[b*G:(b+1)*G, :, :lengths[b]], the rest of the
 *                 row is 0 (an item of fewer than prod(factors) frames: a row of zeros).  Floors as in the strided convolutions: 7 -> 3 -> 1.
 *   decode_items: z[b, :, :4 * lengths[b]] is BIT-IDENTICAL to dmel_quantizer_decode on ids[b:b+1, :, :lengths[b]], the rest is 0.f.
 * Every layer sees the item's own end: the depthwise k = 7 convolutions of the ConvNeXt blocks pad each item with its own zeros, the
 * column-local layers (k2s2 down / up convolutions, pointwise convolutions, FSQ) store zeros behind it.  What z / ids hold at or behind
 * an item's length is never read (NaN or any code there is harmless).  The launches are those of dmel_quantizer_encode_ex /
 * dmel_quantizer_decode plus one that expands the lengths into a per-stage table in the workspace (len, len / 2, len / 4 or len, 2 len,
 * 4 len).  Strict mode (dmel_quantizer_set_strict) applies to encode_items as to encode; prequant / latents are not offered.  workspace:
 * at least dmel_quantizer_items_workspace_bytes(q, B, T) with T in feature frames (= T4 * prod(factors) for decode).  Errors (NULL, handle
 * not finalized, bad B / T, workspace too small) write nothing. */
size_t dmel_quantizer_items_workspace_bytes(const dmel_quantizer* q, int B, int64_t T);
int dmel_quantizer_encode_items(const dmel_quantizer* q, const float* z, const int64_t* lengths_dev, int32_t* ids, int B, int64_t T,
                                void* workspace, size_t workspace_bytes, void* stream);
int dmel_quantizer_decode_items(const dmel_quantizer* q, const int32_t* ids, const int64_t* lengths_dev, float* z, int B, int64_t T4,
                                void* workspace, size_t workspace_bytes, void* stream);
/* Training path of the quantiser: DownsampleFiniteScalarQuantize.forward (dowmsample_fsq.py:86-122) with the straight-through FSQ of
 * vector_quantize_pytorch, and its backward.  z (B*G, Cg, T) -> zq (B*G, Cg, T) (= (B, G*Cg, T); zero-padded from 2^nf * T4 back to T
 * with left = diff / 2), ids (B, G, T4) and latents (B*G, Cg, T4) (both nullable).  Same conventions as the WaveNet training entry
 * points (enable_training before finalize; the workspace of forward_train is handed to backward unchanged; one flat gradient buffer
 * addressed through grad_slot with the state-dict keys).  dz is always produced. */
int dmel_quantizer_enable_training(dmel_quantizer* q, int on);
int dmel_quantizer_set_train_precision(dmel_quantizer* h, int precision);   /* see dmel_wavenet_set_train_precision */
/* as dmel_wavenet_refresh: re-pack every weight image / parameter buffer from device tensors named by their state-dict keys */
int dmel_quantizer_refresh(dmel_quantizer* q, int n, const char* const* keys, const float* const* device_tensors, void* stream);
size_t dmel_quantizer_train_workspace_bytes(const dmel_quantizer* q, int B, int64_t T);
int64_t dmel_quantizer_grad_floats(const dmel_quantizer* q);
int dmel_quantizer_grad_slot(const dmel_quantizer* q, const char* key, int64_t* offset, int64_t* numel);
int dmel_quantizer_forward_train(const dmel_quantizer* q, const float* z, float* zq, int32_t* ids /*nullable*/,
                                 float* latents /*nullable*/, int B, int64_t T, void* workspace, size_t workspace_bytes, void* stream);
int dmel_quantizer_backward(const dmel_quantizer* q, const float* z, const float* dzq, float* dz, float* grads, int B, int64_t T,
                            void* workspace, size_t workspace_bytes, void* stream);

/* z[b,c,t] = z[b,c,t] * (t < lengths[b]) + (w[c] * value + bias[c])      codec_lit_modules.py:520-526
 * (quality_projection = nn.Linear(1, C) applied to the constant 2.0).  w, bias: device (C). */
int dmel_mask_add_quality_f32(float* z, const int64_t* lengths, const float* w, const float* bias, float value,
                              int B, int C, int64_t T, void* stream);

/* The FSQ kernels of the quantiser alone, without the down- / up-sampling stacks around them, on device pointers in the handle's packed
 * layouts: w_in (G, D, C), b_in (G, D), w_out (G, C, D), b_out (G, C), D = n_levels (1..4, host int array `levels`, each 2..1024, product
 * below 2^31).  z / x / dout / dx: (B*G, C, T4) with group g of item b at row b*G + g; ids (B, G, T4) int32; prequant (G, B, T4, D),
 * nullable.  lengths_dev (B device int64, nullable): token counts, clamped into [0, T4] on the device -- ids, prequant (when given) and z
 * at or behind item b's count are written as 0 / 0.f and the z / ids there are not read.  strict: as dmel_quantizer_set_strict.
 *   encode:   ids and prequant = bound(bound?(W_in z + b_in)) (bounded once more first when prebound), rounded half to even.
 *   decode:   z = W_out code + b_out, code_j = (digit_j - levels_j / 2) / (levels_j / 2).
 *   backward: the straight-through estimator; dx and the four parameter gradients (overwritten, not accumulated); scratch: device,
 *             at least 2 * B * G * T4 * D floats.
 * A bad argument (NULL, a shape or level outside the ranges, a scratch too small) is DMEL_EINVAL and writes nothing. */
int dmel_fsq_encode_f32(const float* z, const float* w_in, const float* b_in, const int* levels, int n_levels, int prebound, int strict,
                        const int64_t* lengths_dev /*nullable*/, int32_t* ids, float* prequant /*nullable*/, int B, int G, int C, int64_t T4,
                        void* stream);
int dmel_fsq_decode_f32(const int32_t* ids, const float* w_out, const float* b_out, const int* levels, int n_levels,
                        const int64_t* lengths_dev /*nullable*/, float* z, int B, int G, int C, int64_t T4, void* stream);
int dmel_fsq_backward_f32(const float* x, const float* dout, const float* w_in, const float* b_in, const float* w_out, const int* levels,
                          int n_levels, int prebound, float* dx, float* dw_in, float* db_in, float* dw_out, float* db_out, float* scratch,
                          size_t scratch_floats, int B, int G, int C, int64_t T4, void* stream);

/* BigVGAN generator      replaces models/modules/bigvgan/bigvgan.py:367-393 (+ AMPBlock1 :132-141, AMPBlock2 :232-237) */
typedef struct dmel_bigvgan dmel_bigvgan;
typedef struct dmel_bigvgan_config {
  int num_mels;
  int upsample_initial_channel;
  int num_upsamples;
  int upsample_rates[8];
  int upsample_kernel_sizes[8];
  int num_kernels;
  int resblock_kernel_sizes[8];
  int resblock_dilations[8][3];
  int snake_logscale;      /* h.snake_logscale */
  int activation_snake;    /* 1: "snake", 0: "snakebeta" */
  int use_tanh_at_final;
  int use_bias_at_final;
  int resblock_type;       /* 1 (or 0): AMPBlock1 (bigvgan.py:31-147), 2: AMPBlock2 (bigvgan.py:150-241: per dilation act -> conv -> + x, keys convs.{l}) */
} dmel_bigvgan_config;
int dmel_bigvgan_create(dmel_bigvgan** m, const dmel_bigvgan_config* cfg);
void dmel_bigvgan_destroy(dmel_bigvgan* m);
int dmel_bigvgan_set_tensor(dmel_bigvgan* m, const char* key, const float* data_host, const int64_t* shape, int ndim);
int dmel_bigvgan_finalize(dmel_bigvgan* m);
size_t dmel_bigvgan_workspace_bytes(const dmel_bigvgan* m, int B, int64_t T);
/* Number of streams the AMP blocks of a stage are spread over: 1 = everything on the caller's stream, 3 (default) =
 * caller's stream + two library-owned side streams forked/joined with events inside every stage (the VALU-bound
 * activations of one block then overlap the MFMA-bound convolutions of another).  Results are identical.  A handle's
 * forward is not re-entrant from two host threads at once (it owns the fork/join events). */
int dmel_bigvgan_set_streams(dmel_bigvgan* m, int n_streams);
int dmel_bigvgan_set_precision(dmel_bigvgan* m, int precision);   /* DMEL_PRECISION_*; conv_post (C -> 1) always runs in fp32 */
/* mel (B, num_mels, T) -> audio (B, 1, T * prod(upsample_rates)) */
int dmel_bigvgan_forward(const dmel_bigvgan* m, const float* mel, float* audio, int B, int64_t T,
                         void* workspace, size_t workspace_bytes, void* stream);
/* One pass over mel windows of DIFFERENT lengths (extension: a pool of live sessions whose replies grow by different amounts vocodes
 * all of them at once).  mel (B, num_mels, T) with T the largest window, lengths_dev (B) device int64, 0 <= lengths[b] <= T (clamped on
 * the device; never read by the host, no synchronisation).  audio (B, 1, T * up): audio[b, 0, :lengths[b] * up] is BIT-IDENTICAL to
 * dmel_bigvgan_forward on mel[b:b+1, :, :lengths[b]] -- every layer sees the item's own end: zero padding in the convolutions, replicate
 * padding in the anti-aliased activations -- and the rest of the row is 0 (an item of length 0: a row of zeros).  What mel holds at or
 * beyond an item's length is never read (NaN there is harmless).  The launches are those of dmel_bigvgan_forward plus one that expands
 * the lengths into per-stage tables in the workspace; every precision and both stream settings are served.  The fused act -> conv
 * kernel (DMEL_FUSE_SNAKE) and the producer / consumer convolution have one length per batch and stand aside.  workspace: at least
 * dmel_bigvgan_items_workspace_bytes(m, B, T).  Errors (NULL, handle not finalized, bad B / T, workspace too small) write nothing. */
size_t dmel_bigvgan_items_workspace_bytes(const dmel_bigvgan* m, int B, int64_t T);
int dmel_bigvgan_forward_items(const dmel_bigvgan* m, const float* mel, const int64_t* lengths_dev, float* audio, int B, int64_t T,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Input gradient through the FROZEN generator (bigvgan.py:367-393 under autograd; the reference keeps the vocoder's weights frozen,
 * codec_lit_modules.py:68-72): d loss / d mel from d loss / d audio, for waveform-domain losses on the codec's decoder.  No parameter
 * gradient is produced.
 *   enable_input_grad(m, 1), AFTER finalize, packs the backward-data images (transposed, tap-reversed copies of every convolution: the
 *     vocoder's weight memory doubles); (m, 0) frees them.  A later finalize drops them.
 *   forward_train = dmel_bigvgan_forward with the input of every activation kept in `workspace` (per stage the up-sampled tensor and
 *     per AMP layer its x and conv1 output: 16 tensors per stage with three AMPBlock1s) instead of recycled; always the two-kernel
 *     act -> conv form.  Its audio is bit-identical to dmel_bigvgan_forward's, with one stream and with three.
 *   backward_input must be given the SAME workspace, untouched, and the same B, T: daudio (B, 1, T * up) -> dmel (B, num_mels, T),
 *     overwritten.  Convolutions run their backward-data on the six-product bf16 split; the sum over the AMP blocks of a stage is
 *     taken in block order whatever dmel_bigvgan_set_streams says, so one stream and three give equal bits.
 * Errors (handle not enabled, bad B / T, workspace smaller than dmel_bigvgan_train_workspace_bytes, NULL) write nothing. */
int dmel_bigvgan_enable_input_grad(dmel_bigvgan* m, int on);
size_t dmel_bigvgan_train_workspace_bytes(const dmel_bigvgan* m, int B, int64_t T);
int dmel_bigvgan_forward_train(const dmel_bigvgan* m, const float* mel, float* audio, int B, int64_t T, void* workspace,
                               size_t workspace_bytes, void* stream);
int dmel_bigvgan_backward_input(const dmel_bigvgan* m, const float* daudio, float* dmel, int B, int64_t T, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Discriminator (models/modules/discriminator.py:6-35): six weight-normed Conv2d (3 x 9 | 3 x 3, stride (1, 1|2)) + SiLU over the mel
 * image.  set_tensor keys as in the reference's state dict: blocks.{0,2,..,10}.bias, blocks.{i}.parametrizations.weight.original0|1
 * (weight norm is folded at finalize).  x (B, H = n_mels, W = frames) -> logits (B, H, dmel_discriminator_out_frames(W)).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmel_discriminator dmel_discriminator;
int dmel_discriminator_create(dmel_discriminator** d);
void dmel_discriminator_destroy(dmel_discriminator* d);
int dmel_discriminator_set_tensor(dmel_discriminator* d, const char* key, const float* data_host, const int64_t* shape, int ndim);
int dmel_discriminator_finalize(dmel_discriminator* d);
int64_t dmel_discriminator_out_frames(const dmel_discriminator* d, int64_t W);
size_t dmel_discriminator_workspace_bytes(const dmel_discriminator* d, int B, int H, int64_t W);
int dmel_discriminator_forward(const dmel_discriminator* d, const float* x, float* y, int B, int H, int64_t W, void* workspace,
                               size_t workspace_bytes, void* stream);
/* Training path (same conventions as the WaveNet's): forward_train keeps every layer's input and pre-activation in the workspace,
 * backward returns dx (nullable) and the gradients of bias / weight-norm g (original0) / v (original1) of every layer in the flat
 * buffer (the chain through torch._weight_norm is applied here).  enable_training requires the weight-normed form of the weights. */
int dmel_discriminator_enable_training(dmel_discriminator* d, int on);
int dmel_discriminator_set_train_precision(dmel_discriminator* h, int precision);   /* see dmel_wavenet_set_train_precision */
/* as dmel_wavenet_refresh (keys: blocks.{i}.bias, ...original0, ...original1); the weight-norm fold runs on the device */
int dmel_discriminator_refresh(dmel_discriminator* d, int n, const char* const* keys, const float* const* device_tensors, void* stream);
size_t dmel_discriminator_train_workspace_bytes(const dmel_discriminator* d, int B, int H, int64_t W);
int64_t dmel_discriminator_grad_floats(const dmel_discriminator* d);
int dmel_discriminator_grad_slot(const dmel_discriminator* d, const char* key, int64_t* offset, int64_t* numel);
int dmel_discriminator_forward_train(const dmel_discriminator* d, const float* x, float* y, int B, int H, int64_t W, void* workspace,
                                     size_t workspace_bytes, void* stream);
int dmel_discriminator_backward(const dmel_discriminator* d, const float* dy, float* dx /*nullable*/, float* grads, int B, int H, int64_t W,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Single-op entry point for the implicit-GEMM conv kernel (tests, module mirrors).
 * y = conv1d(x, w, bias, dilation, padding = dilation*(k-1)/2)   w_host: (Cout, Cin, k) as nn.Conv1d stores it.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmel_conv dmel_conv;
int dmel_conv_create(dmel_conv** c, const float* w_host, const float* bias_host /*nullable*/, int Cout, int Cin, int k,
                     int dilation);
void dmel_conv_destroy(dmel_conv* c);
int dmel_conv_set_precision(dmel_conv* c, int precision);
int dmel_conv_forward(const dmel_conv* c, const float* x, float* y, int B, int64_t T, void* stream);
/* dmel_conv_forward with the options of the LINEAR epilogue and of the input staging that the modules use (tests of those paths):
 *   y = (accumulate ? y : 0) + conv1d(x) + bias (+ residual), then / out_div (1.0f: no division).
 * residual (B, Cout, T) nullable.  in_len / out_len: device int64[B], nullable -- input columns at or behind in_len[b] read as zero, output
 * columns at or behind out_len[b] are written as zero.  fold_pitch > 0: the folded batch of short items -- B must be 1, the row holds
 * T / fold_pitch items of fold_valid columns each, followed by fold_pitch - fold_valid zero columns that the caller keeps zero in x; the
 * gap columns of y are written as zero. */
int dmel_conv_forward_ex(const dmel_conv* c, const float* x, float* y, int B, int64_t T, const float* residual /*nullable*/, int accumulate,
                         float out_div, const int64_t* in_len /*nullable*/, const int64_t* out_len /*nullable*/, int fold_pitch, int fold_valid,
                         void* stream);
/* Activation1d fused into the convolution that reads it: y = conv1d(Activation1d(x)) + bias (+ residual), the act -> conv pair of
 * AMPBlock1 / AMPBlock2.forward (bigvgan/bigvgan.py:132-141, :232-237; alias_free_activation/torch/act.py:25-30) as ONE kernel --
 * producer waves compute the anti-aliased Snake of the staged x tile in LDS while consumer waves run the MFMA loop, so the activated
 * tensor never exists in HBM.  x (B, Cin, T) is the tensor BEFORE the activation; alpha / beta (Cin; beta NULL = Snake), filters and
 * logscale as in dmel_aa_snake_f32; residual (B, Cout, T) nullable.  Always computes in DMEL_PRECISION_FP32_F16X2 and is
 * BIT-IDENTICAL to dmel_aa_snake_f32 followed by dmel_conv_forward at that precision.  (k - 1) * dilation <= 64. */
int dmel_conv_snake_forward(const dmel_conv* c, const float* x, const float* residual /*nullable*/, float* y, const float* alpha,
                            const float* beta /*nullable*/, const float* up_filter12_host, const float* down_filter12_host,
                            int logscale, int B, int64_t T, void* stream);
/* Backward of the same convolution -- what autograd runs for the reference (`loss.backward()`, codec_lit_modules.py:236,315 ->
 * ATen conv1d backward); first piece of the training path (SURVEY.md section 8(f) rank 1, C-ABI row `conv1d_dilated(+_bwd)`).
 *   backward_data:   dx (B, Cin, T)  = conv1d(dy, W transposed and tap-reversed)   -- the forward kernel on a second weight image
 *   backward_weight: dw (Cout, Cin, k) = sum_{b,t} dy[b,co,t] * x[b,ci,t + k*d - p], db (Cout) = sum_{b,t} dy   (db nullable)
 * dw / db are overwritten.  The K split of backward_weight uses fp32 atomics: results are reproducible to rounding, not
 * bitwise.  Gradients are always fp32-grade (a BF16 handle falls back to FP32 here). */
int dmel_conv_backward_data(dmel_conv* c, const float* dy, float* dx, int B, int64_t T, void* stream);
int dmel_conv_backward_weight(const dmel_conv* c, const float* x, const float* dy, float* dw, float* db /*nullable*/, int B,
                              int64_t T, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Standalone transposed convolution and output convolution      (convT1d, conv_post)
 * ConvTranspose1d(Cin, Cout, k = 2 * stride, stride, padding = stride / 2): every up-sampler of BigVGAN
 * (models/modules/bigvgan/bigvgan.py:320-334, applied at :371-374), run as `stride` phase sub-convolutions on the implicit-GEMM
 * kernel.  w_host (Cin, Cout, k) and bias_host (Cout, nullable) are HOST arrays in torch's ConvTranspose1d layout, weight norm
 * already folded.  x (B, Cin, T) -> y (B, Cout, T * stride), device, fp32.  Other k / stride / padding: DMEL_EUNSUPPORTED.
 * dmel_conv_post_f32: the C -> 1 convolution that ends the vocoder (bigvgan.py:386-391): y[b, 0, t] = act(bias + sum_{c,k} w[c, k]
 * x[b, c, t + k - K/2]), act 0 none / 2 tanh / 3 clamp to [-1, 1]; w_dev (C, K) DEVICE floats, K odd, C * K * 4 <= 48 KB.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmel_conv_transpose dmel_conv_transpose;
int dmel_conv_transpose1d_create(dmel_conv_transpose** out, const float* w_host, const float* bias_host, int Cin, int Cout, int k, int stride);
void dmel_conv_transpose1d_destroy(dmel_conv_transpose* h);
int dmel_conv_transpose1d_set_precision(dmel_conv_transpose* h, int precision);   /* DMEL_PRECISION_* */
int dmel_conv_transpose1d_forward(const dmel_conv_transpose* h, const float* x, float* y, int B, int64_t T, void* stream);
/* dmel_conv_transpose1d_forward over items: T is the row pitch of x, lengths_dev (B) device int64 in [0, T]; x[b, :, lengths[b]:] reads as
 * zero (it is not read), every one of the T * stride output columns is written.
 * Strides 2, 4 and 8 run as ONE launch: one weight image with all phases (rows channel-major, phase-minor) over the taps d = -1, 0, +1, the
 * tap a phase does not use carrying zeros, so each output keeps the bits of the two phase-group launches; a lane stores 2 or 4 consecutive
 * output samples at once where y and its row pitch are 8- / 16-byte aligned, single floats otherwise (any pointer is accepted).  A zero
 * weight times a non-finite x is NaN: an Inf / NaN sample also reaches the output columns of the neighbouring phase group, which the two
 * launches kept apart.  The one-launch image is packed by the FIRST forward that wants it (a host <-> device copy and a synchronise, under a
 * lock): run one forward before capturing the stream into a graph.  DMEL_UPSTAGE_ONE_LAUNCH=0 (environment, read per call) keeps the two
 * launches. */
int dmel_conv_transpose1d_forward_items(const dmel_conv_transpose* h, const float* x, float* y, int B, int64_t T, const int64_t* lengths_dev,
                                        void* stream);
int dmel_conv_post_f32(const float* x, const float* w_dev, float bias, int act, float* y, int B, int C, int K, int64_t T, void* stream);
/* dmel_conv_post_f32 over items: T is the row pitch, lengths_dev (B) device int64 in [0, T].  Taps at or beyond lengths[b] read as zero
 * (the item's own zero padding; x is not read there), y[b, 0, :lengths[b]] is BIT-IDENTICAL to dmel_conv_post_f32 on the item alone and
 * y[b, 0, lengths[b]:] = 0. */
int dmel_conv_post_items_f32(const float* x, const float* w_dev, float bias, int act, float* y, int B, int C, int K, int64_t T,
                             const int64_t* lengths_dev, void* stream);
/* Backward-data of the two (what autograd runs through F.conv_transpose1d / F.conv1d + tanh | clamp in bigvgan.py:371-374, :386-391):
 *   conv_transpose1d_backward_data: dx[b,ci,q] = sum_co sum_kk W[ci,co,kk] dy[b,co, u q + kk - u/2] (zero outside dy), dy (B, Cout, T * stride)
 *     -> dx (B, Cin, T): a stride-u, 2u-tap convolution of dy on the implicit-GEMM kernel (u strided two-tap segments, two per launch),
 *     six-product split.  The images are packed on the FIRST call, from a host copy of the weights the handle keeps: that call
 *     modifies the handle and must not race with another call on it.
 *   conv_post_backward: dx[b,c,t] = sum_k w[c,k] g[b, t - k + K/2], g = dy * act', act' from the saved OUTPUT y (B, 1, T): tanh 1 - y^2,
 *     clamp 1 where |y| < 1 and 0 where the output was clamped, none 1 (y may then be NULL).  dx (B, C, T) is overwritten. */
int dmel_conv_transpose1d_backward_data(dmel_conv_transpose* h, const float* dy, float* dx, int B, int64_t T, void* stream);
int dmel_conv_post_backward_f32(const float* y, const float* dy, const float* w_dev, int act, float* dx, int B, int C, int K, int64_t T,
                                void* stream);

/* Timing hook used by bench.py: when enabled, every launch of the named kernel family on `stream` is
 * bracketed by hipEvents; dmel_prof_read returns the launch count and total milliseconds since the last reset
 * (synchronises the events it reads).  family: "conv_igemm", "aa_snake", "stft_logmel", "small". */
int dmel_prof_enable(int on);
int dmel_prof_reset(void);
int dmel_prof_read(const char* family, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes);
/* the same plus the matrix-core flops the launches ISSUED for those algorithmic flops (6x under the bf16 split, 3x under the fp16 split,
 * 1x with bf16 operands; 0 for families without a matrix-core kernel): total_flops / (total_issue_flops / dense peak) is the family's
 * matrix-core ceiling */
int dmel_prof_read_ex(const char* family, int64_t* launches, double* total_ms, double* total_flops, double* total_bytes,
                      double* total_issue_flops);

#ifdef __cplusplus
}
#endif
#endif /* DMEL_HIP_H */
