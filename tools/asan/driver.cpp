// Drives the host side of every handle of the C ABI (include/dmel_hip.h) under AddressSanitizer on the fake HIP runtime: create ->
// set_tensor for every state-dict key -> finalize (weight-norm folding, re-tiling into MFMA fragment order, three weight images,
// transposed / training images, mel and chunk tables) -> workspace planning -> forward / training entry points (argument checks, tile
// selection, launch assembly; the kernels themselves do not run).  Exits non-zero on any error return; ASan aborts on any bad access.
// After every module handle's finalize it prints one "uploads <label>: ..." line, the sorted (bytes, FNV-1a) pairs of everything the
// handle uploaded between create and the return of finalize (fake_hip.cpp): tests/test_host_asan.py holds them to a recorded fixture,
// so no byte of a packed weight image moves unnoticed.  Only the handles built under `Fingerprinted` print (the small ones: the line of
// a 20-layer WaveNet is 20 KB).  New handles go at the END of main: the weights are draws of one generator.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/dmel_hip.h"

extern "C" void fake_hip_record_uploads(void);
extern "C" void fake_hip_print_uploads(const char* label);
static bool g_fingerprint = false;
struct Fingerprinted { Fingerprinted() { g_fingerprint = true; } ~Fingerprinted() { g_fingerprint = false; } };
static void record_uploads() { if (g_fingerprint) fake_hip_record_uploads(); }
static void print_uploads(const std::string& l) { if (g_fingerprint) fake_hip_print_uploads(l.c_str()); }
static std::string label(const char* name, std::initializer_list<int> v) {
  std::string s = name;
  for (int x : v) s += "_" + std::to_string(x);
  return s;
}

static std::mt19937 rng(7);
static int failures = 0;
#define CK(call)                                                                                   \
  do {                                                                                             \
    int rc__ = (call);                                                                             \
    if (rc__ != 0) { std::printf("FAIL %s -> %d: %s\n", #call, rc__, dmel_last_error()); ++failures; } \
  } while (0)

template <class H, class F> static void set(H* h, F fn, const std::string& key, std::vector<int64_t> shape, float scale = 0.05f) {
  size_t n = 1;
  for (auto d : shape) n *= (size_t)d;
  std::vector<float> v(n);
  std::normal_distribution<float> nd(0.f, scale);
  for (auto& x : v) x = nd(rng);
  CK(fn(h, key.c_str(), v.data(), shape.data(), (int)shape.size()));
}
static std::vector<float> buf(size_t n) { return std::vector<float>(n + 64, 0.25f); }

static void wavenet(int Cin, int Cout, int C, int L, int cycle, int Cc, int N, int T, bool train) {
  dmel_wavenet* m = nullptr;
  record_uploads();
  CK(dmel_wavenet_create(&m, Cin, Cout, C, L, cycle, Cc));
  if (train) CK(dmel_wavenet_enable_training(m, 1));
  auto S = [&](const std::string& k, std::vector<int64_t> s) { set(m, dmel_wavenet_set_tensor, k, s); };
  if (Cin != C) { S("input_projection.conv.weight", {C, Cin, 1}); S("input_projection.conv.bias", {C}); }
  for (int i = 0; i < L; ++i) {
    const std::string p = "residual_layers." + std::to_string(i) + ".";
    S(p + "conv_layer.conv.weight", {2 * C, C, 3}); S(p + "conv_layer.conv.bias", {2 * C});
    S(p + "output_projection.conv.weight", {2 * C, C, 1}); S(p + "output_projection.conv.bias", {2 * C});
    if (Cc) { S(p + "condition_projection.conv.weight", {2 * C, Cc, 1}); S(p + "condition_projection.conv.bias", {2 * C}); }
  }
  S("skip_projection.conv.weight", {C, C, 1}); S("skip_projection.conv.bias", {C});
  if (Cout != C) { S("output_projection.conv.weight", {Cout, C, 1}); S("output_projection.conv.bias", {Cout}); }
  CK(dmel_wavenet_finalize(m));
  print_uploads(label("wavenet", {Cin, Cout, C, L, cycle, Cc, (int)train}));
  auto x = buf((size_t)N * Cin * T), c = buf((size_t)N * (Cc ? Cc : 1) * T), y = buf((size_t)N * Cout * T);
  std::vector<int64_t> lens(N, T - 1);
  std::vector<char> ws(dmel_wavenet_workspace_bytes(m, N, T) + 256);
  CK(dmel_wavenet_forward(m, x.data(), Cc ? c.data() : nullptr, y.data(), N, T, lens.data(), lens.data(), 1, ws.data(), ws.size(), nullptr));
  for (int prec : {DMEL_PRECISION_BF16, DMEL_PRECISION_FP32_MFMA, DMEL_PRECISION_FP32}) {
    CK(dmel_wavenet_set_precision(m, prec));
    CK(dmel_wavenet_forward(m, x.data(), Cc ? c.data() : nullptr, y.data(), N, T, nullptr, nullptr, 1, ws.data(), ws.size(), nullptr));
  }
  if (train) {
    std::vector<char> tw(dmel_wavenet_train_workspace_bytes(m, N, T) + 256);
    auto dy = buf((size_t)N * Cout * T), dx = buf((size_t)N * Cin * T), dc = buf((size_t)N * (Cc ? Cc : 1) * T);
    auto g = buf((size_t)dmel_wavenet_grad_floats(m));
    CK(dmel_wavenet_forward_train(m, x.data(), Cc ? c.data() : nullptr, y.data(), N, T, tw.data(), tw.size(), nullptr));
    static int64_t covered;
    covered = 0;
    CK(dmel_wavenet_backward_hooked(m, x.data(), Cc ? c.data() : nullptr, dy.data(), dx.data(), Cc ? dc.data() : nullptr, g.data(), N, T,
                                    tw.data(), tw.size(), nullptr, [](void*, int64_t, int64_t n) { covered += n; }, nullptr));
    if (covered != dmel_wavenet_grad_floats(m)) { std::printf("FAIL hook regions cover %lld of %lld\n", (long long)covered, (long long)dmel_wavenet_grad_floats(m)); ++failures; }
    CK(dmel_wavenet_set_train_precision(m, DMEL_PRECISION_BF16));
    CK(dmel_wavenet_forward_train(m, x.data(), Cc ? c.data() : nullptr, y.data(), N, T, tw.data(), tw.size(), nullptr));
  }
  if (Cin == C) {   // incremental forward
    const int64_t cap = 256;
    auto hist = buf((size_t)(L + 1) * N * C * cap), skip = buf((size_t)N * C * cap), cond = buf((size_t)N * (Cc ? Cc : 1) * cap),
         yy = buf((size_t)N * Cout * cap), sc = buf((size_t)2 * N * C * cap);
    std::vector<int64_t> prev(L + 1, 0), next(L + 1);
    next[0] = 200;
    for (int l = 1; l <= L; ++l) next[l] = next[l - 1] - (cycle ? 1 << ((l - 1) % cycle) : 1);
    CK(dmel_wavenet_stream_step(m, hist.data(), skip.data(), Cc ? cond.data() : nullptr, yy.data(), sc.data(), N, cap, prev.data(), next.data(), nullptr));
    prev = next;
    for (int l = 0; l <= L; ++l) next[l] = 230;
    CK(dmel_wavenet_stream_step(m, hist.data(), skip.data(), Cc ? cond.data() : nullptr, yy.data(), sc.data(), N, cap, prev.data(), next.data(), nullptr));
  }
  if (Cin != C && Cout == C && !Cc && C > 32 && C <= 80) {   // encoder side: the step with an input projection, lockstep and per utterance
    const int64_t cap = 256;
    const int G = 2, R = N / G, L1 = L + 1;
    auto xr = buf((size_t)N * Cin * cap), hist = buf((size_t)L1 * N * C * cap), skip = buf((size_t)N * C * cap), yy = buf((size_t)N * C * cap);
    // the scratch of _ex (2 N C cap floats, N int64) followed by the row table of _items ((N / G) * (2 (L + 1) + 1) int32), exactly
    std::vector<float> sc((size_t)2 * N * C * cap + 2 * N + (size_t)R * (2 * L1 + 1));
    std::vector<int64_t> prev(L1, 0), next(L1), lens(R, 190);
    next[0] = 200;
    for (int l = 1; l <= L; ++l) next[l] = std::max<int64_t>(0, next[l - 1] - (cycle ? 1 << ((l - 1) % cycle) : 1));
    CK(dmel_wavenet_stream_step_ex(m, xr.data(), hist.data(), skip.data(), nullptr, yy.data(), sc.data(), N, cap, prev.data(), next.data(),
                                   lens.data(), G, 0, nullptr));
    // rows: 0 mid-stream over several sub-steps, 1 final, 2 idle, the rest mid-stream behind an origin
    std::vector<int64_t> P((size_t)R * L1), Q((size_t)R * L1), O(R, 0);
    for (int r = 0; r < R; ++r)
      for (int l = 0; l <= L; ++l) {
        const int64_t p = next[l], q = r == 1 ? 230 : r == 2 ? p : r == 0 ? p : p + 20;
        P[(size_t)r * L1 + l] = r == 0 ? 0 : p;
        Q[(size_t)r * L1 + l] = q;
        if (r > 2) O[r] = 7;
      }
    auto items = [&]() {
      return dmel_wavenet_stream_step_items(m, xr.data(), hist.data(), skip.data(), nullptr, yy.data(), sc.data(), N, cap, P.data(), Q.data(),
                                            lens.data(), G, O.data(), nullptr);
    };
    CK(items());
    auto refused = [&](const char* what, const char* names) {
      const int rc = items();
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), names)) { std::printf("FAIL stream_step_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
    };
    const auto Q0 = Q;
    if (L >= 2) { Q[(size_t)1 * L1 + 2] = 229; refused("a final row with a level short of the end", "utterance 1"); Q = Q0; }
    Q[(size_t)(R - 1) * L1] = cap + 1; refused("a row past the capacity", R == 2 ? "utterance 1" : "utterance"); Q = Q0;
    if (R > 3) {
      const auto P0 = P;
      for (int l = 0; l <= L; ++l) { Q[(size_t)3 * L1 + l] -= P[(size_t)3 * L1 + L]; P[(size_t)3 * L1 + l] -= P0[(size_t)3 * L1 + L]; }
      refused("a window in front of an origin > 0", "utterance 3");
      P = P0; Q = Q0;
    }
    O[0] = -1; refused("a negative origin", "utterance 0"); O[0] = 0;
    if (dmel_wavenet_stream_step_items(m, xr.data(), hist.data(), skip.data(), nullptr, yy.data(), sc.data(), N + 1, cap, P.data(), Q.data(),
                                       lens.data(), G, O.data(), nullptr) != DMEL_EINVAL) { std::printf("FAIL stream_step_items accepted N %% group_repeat != 0\n"); ++failures; }
  } else if (Cin == C) {   // stacks outside the one-launch kernel have no per-item step
    const int64_t cap = 64;
    auto hist = buf((size_t)(L + 1) * N * C * cap), skip = buf((size_t)N * C * cap), cond = buf((size_t)N * (Cc ? Cc : 1) * cap),
         yy = buf((size_t)N * Cout * cap), sc = buf((size_t)2 * N * C * cap + 2 * N + (size_t)N * (2 * L + 3));
    std::vector<int64_t> z((size_t)N * (L + 1), 0), o(N, 0);
    if ((Cc || Cout != C || C > 80) &&
        dmel_wavenet_stream_step_items(m, nullptr, hist.data(), skip.data(), Cc ? cond.data() : nullptr, yy.data(), sc.data(), N, cap, z.data(),
                                       z.data(), nullptr, 1, o.data(), nullptr) != DMEL_EUNSUPPORTED) {
      std::printf("FAIL stream_step_items took a stack outside the one-launch kernel\n"); ++failures;
    }
  }
  if (Cin == C) {   // any of these stacks per utterance through the LAYERED step: per-item column windows, good and bad tables
    const int64_t cap = 256;
    const int L1 = L + 1, R = N;
    auto hist = buf((size_t)L1 * N * C * cap), skip = buf((size_t)N * C * cap), cond = buf((size_t)N * (Cc ? Cc : 1) * cap),
         yy = buf((size_t)N * Cout * cap);
    std::vector<float> sc((size_t)2 * N * C * cap + 2 * N + (size_t)R * (2 * L1 + 1));
    std::vector<int64_t> F(L1), lens(R, 125);
    F[0] = 100;
    for (int l = 1; l <= L; ++l) F[l] = F[l - 1] - (cycle ? 1 << ((l - 1) % cycle) : 1);
    // rows: 0 the first push from frame 0, 1 mid-stream behind an origin, 2 final, 3 idle
    std::vector<int64_t> P((size_t)R * L1), Q((size_t)R * L1), O(R, 0);
    for (int r = 0; r < R; ++r)
      for (int l = 0; l <= L; ++l) {
        P[(size_t)r * L1 + l] = r % 4 == 0 ? 0 : F[l];
        Q[(size_t)r * L1 + l] = r % 4 == 1 ? F[l] + 20 : r % 4 == 2 ? 130 : F[l];
        if (r % 4 == 1) O[r] = 7;
      }
    auto layered = [&](int n) {
      return dmel_wavenet_stream_step_items_layered(m, nullptr, hist.data(), skip.data(), Cc ? cond.data() : nullptr, yy.data(), sc.data(), n, cap,
                                                    P.data(), Q.data(), lens.data(), 1, O.data(), nullptr);
    };
    CK(dmel_wavenet_set_precision(m, DMEL_PRECISION_FP32));
    CK(layered(N));
    auto refused = [&](const char* what, int code, const char* names) {
      const int rc = layered(N);
      if (rc != code || !std::strstr(dmel_last_error(), names)) { std::printf("FAIL stream_step_items_layered accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
    };
    const auto P0 = P, Q0 = Q;
    if (L >= 2 && R > 1) { Q[(size_t)1 * L1 + 2] = Q[(size_t)1 * L1 + 1]; refused("a level as far as its input", DMEL_EINVAL, "utterance 1"); Q = Q0; }
    Q[(size_t)(R - 1) * L1] = cap + 1; refused("a row past the capacity", DMEL_EINVAL, "utterance"); Q = Q0;
    if (R > 1) {
      for (int l = 0; l <= L; ++l) { Q[(size_t)1 * L1 + l] -= P0[(size_t)1 * L1 + L]; P[(size_t)1 * L1 + l] -= P0[(size_t)1 * L1 + L]; }
      refused("a window in front of an origin > 0", DMEL_EINVAL, "utterance 1");
      P = P0; Q = Q0;
    }
    O[0] = -1; refused("a negative origin", DMEL_EINVAL, "utterance 0"); O[0] = 0;
    for (int prec : {DMEL_PRECISION_BF16, DMEL_PRECISION_FP32_MFMA}) {
      CK(dmel_wavenet_set_precision(m, prec));
      refused("a mode without per-item windows", DMEL_EUNSUPPORTED, "split kernels");
    }
    for (int prec : {DMEL_PRECISION_FP32_F16X2, DMEL_PRECISION_FP32_BF16X3, DMEL_PRECISION_FP32}) {
      CK(dmel_wavenet_set_precision(m, prec));
      CK(layered(N));
    }
    for (auto& v : Q) v = 0;      // every row idle: nothing to launch
    for (auto& v : P) v = 0;
    CK(layered(N));
  }
  dmel_wavenet_destroy(m);
}

static void convnext_keys(const std::string& p, int C, const std::function<void(const std::string&, std::vector<int64_t>)>& S) {
  S(p + "dwconv.weight", {C, 1, 7}); S(p + "dwconv.bias", {C}); S(p + "norm.weight", {C}); S(p + "norm.bias", {C});
  S(p + "pwconv1.weight", {4 * C, C}); S(p + "pwconv1.bias", {4 * C}); S(p + "pwconv2.weight", {C, 4 * C}); S(p + "pwconv2.bias", {C});
  S(p + "gamma", {C});
}

static void quantizer(int G, int C, std::vector<int> levels, int B, int T) {
  dmel_quantizer* q = nullptr;
  int f[2] = {2, 2};
  record_uploads();
  CK(dmel_quantizer_create(&q, G * C, G, levels.data(), (int)levels.size(), f, 2, 1));
  CK(dmel_quantizer_enable_training(q, 1));
  std::function<void(const std::string&, std::vector<int64_t>)> S = [&](const std::string& k, std::vector<int64_t> s) { set(q, dmel_quantizer_set_tensor, k, s); };
  const int D = (int)levels.size();
  for (int i = 0; i < 2; ++i) {
    S("downsample." + std::to_string(i) + ".0.weight", {C, C, 2}); S("downsample." + std::to_string(i) + ".0.bias", {C});
    convnext_keys("downsample." + std::to_string(i) + ".1.", C, S);
    S("upsample." + std::to_string(i) + ".0.weight", {C, C, 2}); S("upsample." + std::to_string(i) + ".0.bias", {C});
    convnext_keys("upsample." + std::to_string(i) + ".1.", C, S);
  }
  for (int g = 0; g < G; ++g) {
    const std::string p = "residual_fsq.rvqs." + std::to_string(g) + ".";
    S(p + "project_in.weight", {D, C}); S(p + "project_in.bias", {D}); S(p + "project_out.weight", {C, D}); S(p + "project_out.bias", {C});
  }
  CK(dmel_quantizer_finalize(q));
  print_uploads(label("quantizer", {G, C, (int)levels.size()}));
  const int T4 = T / 4;
  auto z = buf((size_t)B * G * C * T), zq = buf((size_t)B * G * C * T), pre = buf((size_t)G * B * T4 * D), lat = buf((size_t)B * G * C * T4);
  std::vector<int32_t> ids((size_t)B * G * T4 + 16, 3);
  std::vector<char> ws(dmel_quantizer_workspace_bytes(q, B, T) + 256);
  CK(dmel_quantizer_set_strict(q, 1));
  CK(dmel_quantizer_encode_ex(q, z.data(), ids.data(), pre.data(), lat.data(), B, T, ws.data(), ws.size(), nullptr));
  CK(dmel_quantizer_decode(q, ids.data(), zq.data(), B, T4, ws.data(), ws.size(), nullptr));
  std::vector<char> tw(dmel_quantizer_train_workspace_bytes(q, B, T) + 256);
  auto g = buf((size_t)dmel_quantizer_grad_floats(q));
  CK(dmel_quantizer_forward_train(q, z.data(), zq.data(), ids.data(), lat.data(), B, T, tw.data(), tw.size(), nullptr));
  CK(dmel_quantizer_backward(q, z.data(), zq.data(), z.data(), g.data(), B, T, tw.data(), tw.size(), nullptr));
  dmel_quantizer_destroy(q);
}

static void discriminator(int B, int H, int W) {
  dmel_discriminator* d = nullptr;
  record_uploads();
  CK(dmel_discriminator_create(&d));
  CK(dmel_discriminator_enable_training(d, 1));
  const int cin[6] = {1, 64, 128, 256, 512, 1024}, cout[6] = {64, 128, 256, 512, 1024, 1}, kw[6] = {9, 9, 9, 9, 3, 3};
  for (int i = 0; i < 6; ++i) {
    const std::string p = "blocks." + std::to_string(2 * i) + ".";
    set(d, dmel_discriminator_set_tensor, p + "bias", {cout[i]});
    set(d, dmel_discriminator_set_tensor, p + "parametrizations.weight.original0", {cout[i], 1, 1, 1}, 1.f);
    set(d, dmel_discriminator_set_tensor, p + "parametrizations.weight.original1", {cout[i], cin[i], 3, kw[i]});
  }
  CK(dmel_discriminator_finalize(d));
  print_uploads("discriminator");
  const int64_t Wo = dmel_discriminator_out_frames(d, W);
  auto x = buf((size_t)B * H * W), y = buf((size_t)B * H * Wo), dx = buf((size_t)B * H * W);
  std::vector<char> ws(dmel_discriminator_workspace_bytes(d, B, H, W) + 256), tw(dmel_discriminator_train_workspace_bytes(d, B, H, W) + 256);
  CK(dmel_discriminator_forward(d, x.data(), y.data(), B, H, W, ws.data(), ws.size(), nullptr));
  auto g = buf((size_t)dmel_discriminator_grad_floats(d));
  CK(dmel_discriminator_forward_train(d, x.data(), y.data(), B, H, W, tw.data(), tw.size(), nullptr));
  CK(dmel_discriminator_backward(d, y.data(), dx.data(), g.data(), B, H, W, tw.data(), tw.size(), nullptr));
  dmel_discriminator_destroy(d);
}

static void bigvgan(int n_up, const int* rates, const int* ks, int C0, int mels, int resblock, bool weight_norm, int B, int T) {
  dmel_bigvgan_config c;
  std::memset(&c, 0, sizeof(c));
  c.num_mels = mels; c.upsample_initial_channel = C0; c.num_upsamples = n_up; c.num_kernels = 3;
  const int rk[3] = {3, 7, 11}, rd[3] = {1, 3, 5};
  for (int i = 0; i < n_up; ++i) { c.upsample_rates[i] = rates[i]; c.upsample_kernel_sizes[i] = ks[i]; }
  for (int j = 0; j < 3; ++j) { c.resblock_kernel_sizes[j] = rk[j]; for (int l = 0; l < 3; ++l) c.resblock_dilations[j][l] = rd[l]; }
  c.snake_logscale = 1; c.use_tanh_at_final = 1; c.use_bias_at_final = 1; c.resblock_type = resblock;
  dmel_bigvgan* m = nullptr;
  record_uploads();
  CK(dmel_bigvgan_create(&m, &c));
  auto W = [&](const std::string& p, std::vector<int64_t> shape, bool bias) {
    if (weight_norm) {
      set(m, dmel_bigvgan_set_tensor, p + "weight_g", {shape[0], 1, 1}, 1.f);
      set(m, dmel_bigvgan_set_tensor, p + "weight_v", shape);
    } else {
      set(m, dmel_bigvgan_set_tensor, p + "weight", shape);
    }
    if (bias) set(m, dmel_bigvgan_set_tensor, p + "bias", {p.find("ups.") == 0 ? shape[1] : shape[0]});
  };
  auto A = [&](const std::string& p, int ch) {
    set(m, dmel_bigvgan_set_tensor, p + "act.alpha", {ch}); set(m, dmel_bigvgan_set_tensor, p + "act.beta", {ch});
    set(m, dmel_bigvgan_set_tensor, p + "upsample.filter", {1, 1, 12}); set(m, dmel_bigvgan_set_tensor, p + "downsample.lowpass.filter", {1, 1, 12});
  };
  // all up filters / all down filters must agree: overwrite them with constants afterwards
  W("conv_pre.", {C0, mels, 7}, true);
  int ch = C0;
  for (int i = 0; i < n_up; ++i) {
    W("ups." + std::to_string(i) + ".0.", {C0 >> i, C0 >> (i + 1), ks[i]}, true);
    ch = C0 >> (i + 1);
    for (int j = 0; j < 3; ++j) {
      const std::string bp = "resblocks." + std::to_string(i * 3 + j) + ".";
      for (int l = 0; l < 3; ++l) {
        if (resblock == 2) W(bp + "convs." + std::to_string(l) + ".", {ch, ch, rk[j]}, true);
        else { W(bp + "convs1." + std::to_string(l) + ".", {ch, ch, rk[j]}, true); W(bp + "convs2." + std::to_string(l) + ".", {ch, ch, rk[j]}, true); }
      }
      for (int a = 0; a < (resblock == 2 ? 3 : 6); ++a) {
        set(m, dmel_bigvgan_set_tensor, bp + "activations." + std::to_string(a) + ".act.alpha", {ch});
        set(m, dmel_bigvgan_set_tensor, bp + "activations." + std::to_string(a) + ".act.beta", {ch});
      }
    }
  }
  set(m, dmel_bigvgan_set_tensor, "activation_post.act.alpha", {ch}); set(m, dmel_bigvgan_set_tensor, "activation_post.act.beta", {ch});
  W("conv_post.", {1, ch, 7}, true);
  (void)A;
  CK(dmel_bigvgan_finalize(m));
  print_uploads(label("bigvgan", {n_up, C0, mels, resblock, (int)weight_norm}));
  int up = 1;
  for (int i = 0; i < n_up; ++i) up *= rates[i];
  auto mel = buf((size_t)B * mels * T), y = buf((size_t)B * T * up);
  std::vector<char> ws(dmel_bigvgan_workspace_bytes(m, B, T) + 256);
  for (int streams : {1, 3}) {
    CK(dmel_bigvgan_set_streams(m, streams));
    CK(dmel_bigvgan_forward(m, mel.data(), y.data(), B, T, ws.data(), ws.size(), nullptr));
  }
  CK(dmel_bigvgan_set_precision(m, DMEL_PRECISION_BF16));
  CK(dmel_bigvgan_forward(m, mel.data(), y.data(), B, T, ws.data(), ws.size(), nullptr));
  dmel_bigvgan_destroy(m);
}

int main() {
  // single convolutions: ragged channel counts, every tap count / dilation of the vocoder, forward + both backward entry points
  const int shapes[][6] = {{256, 256, 7, 3, 736, 2}, {128, 128, 11, 5, 3000, 1}, {1120, 560, 3, 2, 92, 2}, {70, 10, 1, 1, 93, 5}, {33, 17, 3, 1, 50, 1},
                           {32, 32, 3, 1, 23552, 1}, {100, 560, 1, 1, 92, 3}, {128, 64, 9, 1, 4592, 2}, {96, 80, 3, 1, 700, 2}};
  for (auto& s : shapes) {
    const int Cout = s[0], Cin = s[1], k = s[2], dil = s[3], T = s[4], B = s[5];
    std::vector<float> w((size_t)Cout * Cin * k, 0.01f), b(Cout, 0.1f);
    dmel_conv* c = nullptr;
    CK(dmel_conv_create(&c, w.data(), b.data(), Cout, Cin, k, dil));
    auto x = buf((size_t)B * Cin * T), y = buf((size_t)B * Cout * T), dw = buf((size_t)Cout * Cin * k), db = buf(Cout);
    for (int prec : {DMEL_PRECISION_FP32, DMEL_PRECISION_BF16, DMEL_PRECISION_FP32_MFMA, DMEL_PRECISION_FP32_F16X2, DMEL_PRECISION_FP32_BF16X3}) {
      CK(dmel_conv_set_precision(c, prec));
      CK(dmel_conv_forward(c, x.data(), y.data(), B, T, nullptr));
    }
    CK(dmel_conv_backward_data(c, y.data(), x.data(), B, T, nullptr));
    CK(dmel_conv_backward_weight(c, x.data(), y.data(), dw.data(), db.data(), B, T, nullptr));
    dmel_conv_destroy(c);
  }
  wavenet(10, 70, 70, 20, 4, 0, 16, 93, true);          // encoder (whole-stack kernel table)
  wavenet(48, 48, 48, 3, 4, 0, 4, 17, false);
  wavenet(560, 80, 560, 4, 4, 560, 3, 92, true);        // decoder (conditioned, output projection, XCD-chunked grids, streaming)
  wavenet(64, 64, 64, 5, 0, 64, 2, 40, false);
  quantizer(8, 70, {7, 5, 5}, 3, 93);
  { Fingerprinted fp; quantizer(2, 70, {8, 6}, 2, 47); }
  {
    dmel_convnext* cx = nullptr;
    record_uploads();
    CK(dmel_convnext_create(&cx, 70));
    CK(dmel_convnext_enable_training(cx, 1));
    std::function<void(const std::string&, std::vector<int64_t>)> S = [&](const std::string& k, std::vector<int64_t> s) { set(cx, dmel_convnext_set_tensor, k, s); };
    convnext_keys("", 70, S);
    CK(dmel_convnext_finalize(cx));
    print_uploads("convnext_70");
    const int N = 6, T = 46;
    auto x = buf((size_t)N * 70 * T), y = buf((size_t)N * 70 * T), g = buf((size_t)dmel_convnext_grad_floats(cx));
    std::vector<char> ws(dmel_convnext_workspace_bytes(cx, N, T) + 256), tw(dmel_convnext_train_workspace_bytes(cx, N, T) + 256);
    CK(dmel_convnext_forward(cx, x.data(), y.data(), N, T, ws.data(), ws.size(), nullptr));
    CK(dmel_convnext_forward_train(cx, x.data(), y.data(), N, T, tw.data(), tw.size(), nullptr));
    CK(dmel_convnext_backward(cx, x.data(), y.data(), x.data(), g.data(), N, T, tw.data(), tw.size(), nullptr));
    dmel_convnext_destroy(cx);
  }
  discriminator(2, 80, 93);
  { Fingerprinted fp; discriminator(1, 16, 60); }
  { const int r[4] = {8, 8, 2, 2}, k[4] = {16, 16, 4, 4}; bigvgan(4, r, k, 512, 80, 1, true, 2, 12); }
  { Fingerprinted fp; const int r[2] = {4, 2}, k[2] = {8, 4}; bigvgan(2, r, k, 32, 20, 2, false, 2, 9); }
  { const int r[6] = {4, 4, 2, 2, 2, 2}, k[6] = {8, 8, 4, 4, 4, 4}; bigvgan(6, r, k, 96, 100, 1, true, 1, 3); }
  {   // standalone transposed convolution / output convolution
    for (int stride : {2, 8}) {
      const int Ci = 40, Co = 24, k = 2 * stride, B = 2, T = 37;
      std::vector<float> w((size_t)Ci * Co * k, 0.02f), b(Co, 0.1f);
      dmel_conv_transpose* h = nullptr;
      CK(dmel_conv_transpose1d_create(&h, w.data(), b.data(), Ci, Co, k, stride));
      auto x = buf((size_t)B * Ci * T), y = buf((size_t)B * Co * T * stride);
      for (int prec : {DMEL_PRECISION_FP32, DMEL_PRECISION_FP32_F16X2, DMEL_PRECISION_BF16}) {
        CK(dmel_conv_transpose1d_set_precision(h, prec));
        CK(dmel_conv_transpose1d_forward(h, x.data(), y.data(), B, T, nullptr));
      }
      dmel_conv_transpose1d_destroy(h);
    }
    dmel_conv_transpose* bad = nullptr;
    if (dmel_conv_transpose1d_create(&bad, buf(64).data(), nullptr, 4, 4, 3, 2) == 0) { std::printf("FAIL conv_transpose1d accepted k != 2 stride\n"); ++failures; }
    auto xp = buf(3 * 32 * 500), wp = buf(32 * 7), yp = buf(3 * 500);
    CK(dmel_conv_post_f32(xp.data(), wp.data(), 0.3f, 2, yp.data(), 3, 32, 7, 500, nullptr));
  }
  for (int nfft : {512, 1024, 2048}) {
    dmel_stft_plan* p = nullptr;
    CK(dmel_stft_plan_create(&p, nfft == 2048 ? 44100 : 24000, nfft, nfft, nfft / 4, nfft == 2048 ? 128 : 80, 0.0, 0.0, nullptr));
    const int B = 2; const int64_t L = 24000;
    auto a = buf((size_t)B * L);
    const int64_t T = dmel_stft_num_frames(p, L);
    auto mel = buf((size_t)B * 128 * T), lin = buf((size_t)B * T * (nfft / 2 + 1));
    CK(dmel_stft_logmel_f32(p, a.data(), L, nullptr, mel.data(), B, L, nullptr));
    CK(dmel_stft_f32(p, a.data(), L, nullptr, nullptr, lin.data(), B, L, nullptr));
    {   // windows of longer signals: one for the whole batch, then one per item
      const int hop = nfft / 4, pad = (nfft - hop) / 2;
      const int64_t f0 = 6, nf = 7, s0 = f0 * hop - pad, n = (f0 + nf - 1) * hop - pad + nfft - s0;
      CK(dmel_stft_window_f32(p, a.data(), L, n, s0, nullptr, mel.data(), nullptr, B, f0, nf, -1, nullptr));
      // item 0: the head of a stream (left reflection), its row only partly valid; item 1: the tail of a signal of 9000 samples
      const int64_t Lt = 9000, Tt = dmel_stft_num_frames(p, Lt);
      int64_t S0[2] = {0, (Tt - 3) * hop - pad}, F0[2] = {0, Tt - 3}, NF[2] = {5, 3}, TL[2] = {-1, Lt};
      int64_t NV[2] = {4 * hop - pad + nfft, Lt - S0[1]};
      const int64_t width = std::max(NV[0], NV[1]);
      std::vector<int64_t> tab(8);      // exactly the 4 B int64 the header asks for
      CK(dmel_stft_window_items_f32(p, a.data(), L, width, S0, NV, nullptr, mel.data(), lin.data(), B, F0, NF, TL, tab.data(), nullptr));
      NF[0] = 0;                        // an idle item
      CK(dmel_stft_window_items_f32(p, a.data(), L, width, S0, NV, nullptr, mel.data(), nullptr, B, F0, NF, TL, tab.data(), nullptr));
      NF[0] = 5; NV[0] -= 1;            // item 0's last frame reads a sample its row does not hold
      int rc = dmel_stft_window_items_f32(p, a.data(), L, width, S0, NV, nullptr, mel.data(), nullptr, B, F0, NF, TL, tab.data(), nullptr);
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "item 0")) { std::printf("FAIL stft_window_items accepted a row that misses a sample (%d: %s)\n", rc, dmel_last_error()); ++failures; }
      NV[0] += 1; NF[1] = 4;            // item 1: a frame past the last frame of its signal
      rc = dmel_stft_window_items_f32(p, a.data(), L, width, S0, NV, nullptr, mel.data(), nullptr, B, F0, NF, TL, tab.data(), nullptr);
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "item 1")) { std::printf("FAIL stft_window_items accepted frames past the end (%d: %s)\n", rc, dmel_last_error()); ++failures; }
      NF[1] = 3; NV[1] = width + 1;     // more valid samples than the buffer is wide
      if (dmel_stft_window_items_f32(p, a.data(), L, width, S0, NV, nullptr, mel.data(), nullptr, B, F0, NF, TL, tab.data(), nullptr) != DMEL_EINVAL) { std::printf("FAIL stft_window_items accepted n_valid > n_samples\n"); ++failures; }
    }
    std::vector<float> basis((size_t)128 * (nfft / 2 + 1));
    CK(dmel_stft_plan_mel_basis(p, basis.data()));
    dmel_stft_plan_destroy(p);
  }
  {
    auto x = buf(3 * 5000), y = buf(3 * 7500), bank = buf(3 * 16), al = buf(8), be = buf(8), taps = buf(12);
    CK(dmel_resample_f32(x.data(), y.data(), bank.data(), 3, 5000, 7500, 2, 3, 7, nullptr));
    // outputs [100, 1100) of a stream whose samples [50, 850) are in the buffer: they read [(100 / 3) * 2 - 7, (1099 / 3) * 2 + 9) = [59, 741)
    CK(dmel_resample_window_f32(x.data(), 5000, 800, 50, y.data(), bank.data(), 3, 100, 1000, -1, 2, 3, 7, nullptr));
    if (dmel_resample_window_f32(x.data(), 5000, 800, 60, y.data(), bank.data(), 3, 100, 1000, -1, 2, 3, 7, nullptr) == 0) { std::printf("FAIL resample_window accepted a buffer that misses a tap\n"); ++failures; }
    {   // three streams at two rates in one call: 2 -> 3 (width 7, 3 x 16 taps at arena offset 0) and 3 -> 2 (width 10, 2 x 23 at 48)
      auto arena = buf(48 + 46);
      int64_t RT[8] = {0, 2, 3, 7, 48, 3, 2, 10};
      // item 0: outputs [100, 1100) of samples [50, 850), as above; item 1: the head of a 3 -> 2 stream, outputs [0, 300) read [-10, 460);
      // item 2: the end of a 3 -> 2 signal of 900 samples, outputs [500, 600) read [740, 900) and zeros behind
      int64_t S0[3] = {50, 0, 700}, NV[3] = {800, 460, 200}, O0[3] = {100, 0, 500}, NO[3] = {1000, 300, 100}, TL[3] = {-1, -1, 900};
      int64_t YO[3] = {6500, 10, 0}, RI[3] = {0, 1, 1};
      std::vector<int64_t> tab(7 * 3 + 4 * 2);      // exactly the 7 B + 4 n_rates int64 the header asks for
      auto items = [&]() {
        return dmel_resample_window_items_f32(x.data(), 5000, 800, S0, NV, y.data(), 7500, YO, arena.data(), 94, RT, 2, RI, 3, O0, NO, TL,
                                              tab.data(), nullptr);
      };
      CK(items());
      NV[1] = 459;                        // item 1's last output reads a sample its row does not hold
      int rc = items();
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "item 1")) { std::printf("FAIL resample_window_items accepted a row that misses a tap (%d: %s)\n", rc, dmel_last_error()); ++failures; }
      NV[1] = 460; YO[0] = 6501;          // item 0's outputs run over the end of its output row
      rc = items();
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "item 0")) { std::printf("FAIL resample_window_items accepted a y_off overflow (%d: %s)\n", rc, dmel_last_error()); ++failures; }
      YO[0] = 6500; NO[0] = NO[1] = NO[2] = 0;      // every item idle: nothing to check, nothing to launch
      RI[0] = 7; NV[1] = 9000;
      CK(items());
    }
    {
      // the ragged convert-copy: three items in the three directions, tables of exactly B entries, a table scratch of exactly 4 B int64
      std::vector<float> f(5000, 0.5f), g(2049);
      std::vector<int16_t> p(2049), q(5000);
      const void* SRC[3] = {f.data(), p.data(), f.data()};
      void* DST[3] = {q.data(), g.data(), g.data()};
      int32_t SF[3] = {DMEL_SAMPLE_F32, DMEL_SAMPLE_S16, DMEL_SAMPLE_F32}, DF[3] = {DMEL_SAMPLE_S16, DMEL_SAMPLE_F32, DMEL_SAMPLE_F32};
      int64_t N[3] = {5000, 2049, 0};
      std::vector<int64_t> tab(4 * 3);
      auto conv = [&]() { return dmel_pcm_convert_items(SRC, SF, DST, DF, N, 3, tab.data(), nullptr); };
      CK(conv());
      DF[1] = DMEL_SAMPLE_S16;
      int rc = conv();
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "item 1")) { std::printf("FAIL pcm_convert_items accepted s16 -> s16 (%d: %s)\n", rc, dmel_last_error()); ++failures; }
      DF[1] = DMEL_SAMPLE_F32; SRC[1] = reinterpret_cast<const char*>(p.data()) + 1;
      rc = conv();
      if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "item 1")) { std::printf("FAIL pcm_convert_items accepted an odd s16 pointer (%d: %s)\n", rc, dmel_last_error()); ++failures; }
      N[0] = N[1] = 0; SRC[0] = nullptr;          // every item idle: pointers are not looked at, nothing to launch
      CK(conv());
    }
    {
      // the state fork: its refusals read the host tables only (R entries each), and a step of idle rows launches nothing
      const int Lf = 2, Nf = 6, Cf = 5, Cc = 3, Co = 2;
      const int64_t capf = 96;
      auto hist = buf((size_t)(Lf + 1) * Nf * Cf * capf), skip = buf((size_t)Nf * Cf * capf), cond = buf((size_t)Nf * Cc * capf), mel = buf((size_t)Nf * Co * capf);
      std::vector<int32_t> tab(5 * 2);            // exactly the 5 R int32 the header asks for
      int64_t SRC[2] = {0, 1}, DST[2] = {3, 4}, LO[2] = {0, 4}, HI[2] = {8, 40};
      auto fork = [&]() {
        return dmel_stream_fork_items(hist.data(), skip.data(), cond.data(), mel.data(), Lf, Nf, Cf, Cc, Co, capf, 2, SRC, DST, LO, HI, tab.data(), nullptr);
      };
      auto refused = [&](const char* what) {
        const int rc = fork();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), "row 1")) { std::printf("FAIL stream_fork_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      DST[1] = 1; refused("a row forked into itself");
      DST[1] = 3; refused("two rows with one destination");
      DST[1] = 0; refused("a destination that is a source");
      DST[1] = 6; refused("an item outside [0, N)");
      DST[1] = 4; HI[1] = 97; refused("a window behind cap");
      HI[1] = 40; LO[1] = 41; refused("a window that ends in front of its start");
      LO[0] = HI[0] = 8; LO[1] = HI[1] = 40;      // every row idle
      CK(fork());
    }
    {
      // the cross-fade: tables of exactly R entries, a table scratch of exactly 5 R int64; its refusals read the host tables only
      auto wav = buf(4096), tails = buf(2 * 512), wts = buf(512);
      float* BL[2] = {wav.data() + 256, wav.data() + 1024};
      float* TA[2] = {tails.data(), tails.data() + 512};
      const float* SA[2] = {wav.data() + 768, nullptr};
      const float* WT[2] = {wts.data(), wts.data()};
      int64_t FA[2] = {512, 255};
      std::vector<int64_t> tab(5 * 2);
      auto fade = [&](int R) { return dmel_crossfade_items(BL, TA, SA, WT, FA, R, tab.data(), nullptr); };
      CK(fade(2));
      auto refused = [&](int R, const char* row, const char* what) {
        const int rc = fade(R);
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), row)) { std::printf("FAIL crossfade_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      refused(0, "0 rows", "no row");
      refused(65536, "65536 rows", "more than 65535 rows");
      FA[1] = 0; refused(2, "row 1", "a fade of 0 samples");
      FA[1] = 4097; refused(2, "row 1", "a fade of 4097 samples");
      FA[1] = 255; TA[1] = nullptr; refused(2, "row 1", "a NULL tail");
      TA[1] = tails.data() + 512; WT[0] = nullptr; refused(2, "row 0", "NULL weights");
      WT[0] = wts.data(); BL[1] = nullptr; refused(2, "row 1", "a row with neither blend nor save");
      SA[1] = wav.data() + 2048;                  // a row that only saves
      CK(fade(2));
    }
    {
      // the ragged pack: tables of exactly R entries, a table scratch of exactly 8 R int64; its refusals read the host tables only
      auto state = buf(5 * 99 + 8), blob = buf(5 * 33 + 40);
      const void* SRC[2] = {state.data() + 1, state.data()};
      void* DST[2] = {blob.data(), blob.data() + 5 * 33};
      int64_t RW[2] = {5, 1}, CL[2] = {33, 40}, SP[2] = {99, 0}, DP[2] = {33, 0};
      std::vector<int64_t> tab(8 * 2);
      auto pack = [&](int R) { return dmel_stream_pack_items(SRC, DST, RW, CL, SP, DP, R, tab.data(), nullptr); };
      CK(pack(2));
      auto refused = [&](int R, const char* row, const char* what) {
        const int rc = pack(R);
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), row)) { std::printf("FAIL stream_pack_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      refused(0, "0 rows", "no row");
      refused(65536, "65536 rows", "more than 65535 rows");
      RW[1] = -1; refused(2, "row 1", "a negative row count");
      RW[1] = 1; CL[1] = -40; refused(2, "row 1", "a negative word count");
      CL[1] = 40; SRC[1] = nullptr; refused(2, "row 1", "a NULL source");
      SRC[1] = state.data(); DST[0] = nullptr; refused(2, "row 0", "a NULL destination");
      DST[0] = reinterpret_cast<char*>(blob.data()) + 2; refused(2, "row 0", "a destination that is not 4-byte aligned");
      DST[0] = blob.data(); SP[0] = 32; refused(2, "row 0", "a source pitch below cols");
      SP[0] = 99; DP[0] = 32; refused(2, "row 0", "a destination pitch below cols");
      DP[0] = 33; RW[0] = (int64_t)1 << 34; SP[0] = (int64_t)1 << 6; refused(2, "row 0", "rows * pitch of 2^40");
      RW[0] = (int64_t)1 << 33; CL[0] = 1; SP[0] = (int64_t)1 << 30; refused(2, "row 0", "rows * pitch of 2^63, which wraps as an int64 product");
      SP[0] = 99; DP[0] = (int64_t)1 << 30; refused(2, "row 0", "rows * destination pitch of 2^63");
      CL[0] = 33; DP[0] = 33;
      RW[0] = 0; CL[1] = 0; SRC[0] = nullptr; DST[1] = nullptr; SP[0] = DP[0] = -1;   // every row idle: pointers and pitches are not looked at
      CK(pack(2));
    }
    {
      // the voice detector: tables of exactly S entries (5 S parameters each), a table scratch of exactly 12 S words; its refusals read
      // the host tables only
      const int NM = 80, T = 130;
      auto mel = buf(3 * NM * T), st = buf(3 * (NM + 8));
      std::vector<uint8_t> fl(3 * T), ct(3 * T);
      int64_t NF[3] = {T, 0, 65};
      float FP[15] = {1.5f, -10.f, 0.1f, 0.02f, 0.002f, NAN, NAN, NAN, NAN, NAN, 1.5f, -10.f, 1.f, 1.f, 0.f};
      int32_t IP[15] = {0, NM, 4, 3, 47, -9, -9, -9, -9, -9, 3, 9, 6, 1, 1 << 20};      // the idle item's parameters are not looked at
      std::vector<uint32_t> tab(12 * 3);
      int nm = NM, S = 3;
      int64_t pitch = T;
      auto scan = [&]() { return dmel_voice_items(mel.data(), (int64_t)NM * T, T, nm, S, NF, FP, IP, st.data(), fl.data(), ct.data(), pitch, tab.data(), nullptr); };
      CK(scan());
      auto refused = [&](const char* item, const char* what) {
        const int rc = scan();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL voice_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = 65536; refused("65536 items", "more than 65535 items");
      S = 3; nm = 0; refused("0 mel bands", "no band");
      nm = 129; refused("129 mel bands", "more than 128 bands");
      nm = NM; NF[2] = -1; refused("item 2", "a negative frame count");
      NF[2] = T + 1; refused("item 2", "more frames than the output pitch");
      NF[2] = 65; FP[10] = 0.f; refused("item 2", "a threshold of 0");
      FP[10] = 1.5f; FP[1] = INFINITY; refused("item 0", "a min_level that is not finite");
      FP[1] = -10.f; FP[2] = 0.f; refused("item 0", "fall = 0");
      FP[2] = 0.1f; FP[13] = 1.5f; refused("item 2", "rise above 1");
      FP[13] = 1.f; FP[4] = -0.1f; refused("item 0", "a negative rise_speech");
      FP[4] = 0.002f; IP[1] = NM + 1; refused("item 0", "a band window behind n_mels");
      IP[1] = NM; IP[10] = 9; refused("item 2", "an empty band window");
      IP[10] = 3; IP[12] = 7; refused("item 2", "min_bands above the window");
      IP[12] = 6; IP[3] = 0; refused("item 0", "attack_frames = 0");
      IP[3] = 3; IP[14] = (1 << 20) + 1; refused("item 2", "release_frames above 2^20");
      IP[14] = 1 << 20;
      NF[0] = NF[2] = 0;                          // every item idle
      CK(scan());
    }
    {
      // the DTMF detector: tables of exactly S entries (8 S coefficients, 5 S and 2 S parameters), a table scratch of exactly 20 S words;
      // its refusals read the host tables only
      const int W = 9000;
      auto smp = buf(3 * W), st = buf(3 * 128);
      std::vector<uint8_t> dec(3 * 90), prs(3 * 90);
      int64_t FI[3] = {5, -7, 1}, NN[3] = {8995, 0, 32 * 90};
      int32_t BL[3] = {102, -1, 32};                  // the idle item's parameters are not looked at
      float CO[24], FP[15] = {1.02e-4f, 6.f, 2.51f, 6.31f, 25.5f, NAN, NAN, NAN, NAN, NAN, 3.2e-5f, 6.f, 2.51f, 6.31f, 8.f};
      for (int k = 0; k < 24; ++k) CO[k] = (k >= 8 && k < 16) ? NAN : 2.f - 0.5f * (float)(k % 8);
      int32_t IP[6] = {2, 2, -9, -9, 1, 1 << 20};
      std::vector<uint32_t> tab(20 * 3);
      int S = 3;
      int64_t pitch = 90;
      auto scan = [&]() { return dmel_dtmf_items(smp.data(), W, S, FI, NN, BL, CO, FP, IP, st.data(), dec.data(), prs.data(), pitch, tab.data(), nullptr); };
      CK(scan());
      auto refused = [&](const char* item, const char* what) {
        const int rc = scan();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL dtmf_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = 65536; refused("65536 items", "more than 65535 items");
      S = 3; NN[2] = -1; refused("item 2", "a negative sample count");
      NN[2] = 32 * 90 + 1; refused("item 2", "more blocks than the output pitch");
      NN[2] = 32 * 90; FI[0] = -1; refused("item 0", "a negative first column");
      FI[0] = 5; BL[2] = 31; refused("item 2", "a block of 31 samples");
      BL[2] = 32; BL[0] = 4097; refused("item 0", "a block of 4097 samples");
      BL[0] = 102; CO[17] = 2.5f; refused("item 2", "a coefficient above 2");
      CO[17] = 1.5f; FP[0] = 0.f; refused("item 0", "emin = 0");
      FP[0] = 1.02e-4f; FP[11] = INFINITY; refused("item 2", "a rel that is not finite");
      FP[11] = 6.f; FP[14] = -8.f; refused("item 2", "a negative g");
      FP[14] = 8.f; IP[0] = 0; refused("item 0", "hits = 0");
      IP[0] = 2; IP[5] = (1 << 20) + 1; refused("item 2", "misses above 2^20");
      IP[5] = 1 << 20;
      NN[0] = NN[2] = 0;                          // every item idle
      CK(scan());
    }
    {
      // the input leveller: tables of exactly S entries (10 S parameters), a table scratch of exactly 16 S words; its refusals read
      // the host tables only
      const int W = 9000;
      auto smp = buf(3 * W), st = buf(3 * 16), pk = buf(3 * 90), gn = buf(3 * 90);
      int64_t FI[3] = {5, -7, 1}, NN[3] = {8995, 0, 32 * 90};
      int32_t BL[3] = {240, -1, 32};                  // the idle item's parameters are not looked at
      float FP[30];
      const float good[10] = {1.f, 0.5f, 0.5f / 31.6f, 0.1f, 31.6f, 1.f, 0.02f, 0.003f, 1.f, 1.f / 240.f};
      for (int k = 0; k < 30; ++k) FP[k] = (k >= 10 && k < 20) ? NAN : good[k % 10];
      FP[27] = 0.f; FP[29] = 1.f / 32.f;              // a gate of 0 is allowed
      std::vector<uint32_t> tab(16 * 3);
      int S = 3;
      int64_t pitch = 90;
      auto scan = [&]() { return dmel_level_items(smp.data(), W, S, FI, NN, BL, FP, st.data(), pk.data(), gn.data(), pitch, tab.data(), nullptr); };
      CK(scan());
      auto refused = [&](const char* item, const char* what) {
        const int rc = scan();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL level_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = 65536; refused("65536 items", "more than 65535 items");
      S = 3; NN[2] = -1; refused("item 2", "a negative sample count");
      NN[2] = 32 * 90 + 1; refused("item 2", "more blocks than the output pitch");
      NN[2] = 32 * 90; FI[0] = -1; refused("item 0", "a negative first column");
      FI[0] = 5; BL[2] = 31; refused("item 2", "a block of 31 samples");
      BL[2] = 32; BL[0] = 4097; refused("item 0", "a block of 4097 samples");
      BL[0] = 240; FP[1] = 0.f; refused("item 0", "a target of 0");
      FP[1] = 0.5f; FP[22] = INFINITY; refused("item 2", "an emin that is not finite");
      FP[22] = 0.5f / 31.6f; FP[27] = -0.003f; refused("item 2", "a negative gate");
      FP[27] = 0.f; FP[5] = 1.5f; refused("item 0", "attack above 1");
      FP[5] = 1.f; FP[26] = 2.f; refused("item 2", "release above 1");
      FP[26] = 0.02f; FP[20] = 40.f; refused("item 2", "initial_gain above max_gain");
      FP[20] = 1.f; FP[3] = 2.f; refused("item 0", "min_gain above initial_gain");
      FP[3] = 0.1f;
      NN[0] = NN[2] = 0;                          // every item idle
      CK(scan());
    }
    {
      // the noise suppressor: tables of exactly S entries (8 S parameters), a table scratch of exactly 16 S words, a transform table
      // of exactly 3072 words; its refusals read the host tables only
      const int W = 9000;
      auto smp = buf(3 * W), st = buf(3 * 3092), pi = buf(3 * 90), po = buf(3 * 90), tr = buf(3072);
      int64_t FI[3] = {5, -7, 1}, NN[3] = {8995, 0, 32 * 90};
      int32_t FR[3] = {512, -1, 64}, LF[3] = {16, -1, 1};   // the idle item's parameters are not looked at
      float FP[24];
      const float good[8] = {0.96f, 0.04f, 0.05f, 6.f, 1.002f, 0.126f, 1e-20f, 1.f / 512.f};
      for (int k = 0; k < 24; ++k) FP[k] = (k >= 8 && k < 16) ? NAN : good[k % 8];
      FP[16] = 0.f; FP[17] = 1.f; FP[23] = 1.f / 64.f;      // an alpha of 0 is allowed
      std::vector<uint32_t> tab(16 * 3);
      int S = 3;
      int64_t pitch = 90;
      auto scan = [&]() {
        return dmel_denoise_items(smp.data(), W, S, FI, NN, FR, LF, FP, st.data(), pi.data(), po.data(), pitch, tr.data(), tab.data(), nullptr);
      };
      CK(scan());
      auto refused = [&](const char* item, const char* what) {
        const int rc = scan();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL denoise_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = 65536; refused("65536 items", "more than 65535 items");
      S = 3; NN[2] = -1; refused("item 2", "a negative sample count");
      NN[2] = 32 * 90 + 1; refused("item 2", "more frames than the output pitch");
      NN[2] = 32 * 90; FI[0] = -1; refused("item 0", "a negative first column");
      FI[0] = 5; FR[2] = 32; refused("item 2", "a frame of 32 samples");
      FR[2] = 96; refused("item 2", "a frame that is no power of two");
      FR[2] = 64; FR[0] = 2048; refused("item 0", "a frame of 2048 samples");
      FR[0] = 512; LF[0] = 0; refused("item 0", "learn_frames = 0");
      LF[0] = 16; LF[2] = 4097; refused("item 2", "learn_frames above 4096");
      LF[2] = 1; FP[0] = 1.f; refused("item 0", "an alpha of 1");
      FP[0] = 0.96f; FP[17] = 0.f; refused("item 2", "1 - alpha = 0");
      FP[17] = 1.f; FP[2] = 1.5f; refused("item 0", "a track above 1");
      FP[2] = 0.05f; FP[19] = 0.5f; refused("item 2", "a track_ratio below 1");
      FP[19] = 6.f; FP[4] = INFINITY; refused("item 0", "a creep that is not finite");
      FP[4] = 1.002f; FP[21] = 0.f; refused("item 2", "a floor_gain of 0");
      FP[21] = 0.126f; FP[6] = -1e-20f; refused("item 0", "a negative eps");
      FP[6] = 1e-20f; FP[23] = 1.f / 512.f; refused("item 2", "an rN that is not 1 / N");
      FP[23] = 1.f / 64.f;
      NN[0] = NN[2] = 0;                          // every item idle
      CK(scan());
    }
    {
      // packet-loss concealment: tables of exactly S entries (16 ranges, 6 and 4 parameters each), a table scratch of exactly 48 S
      // words, out rows of exactly the ranges' count; its refusals read the host tables only
      const int W = 9000;
      auto smp = buf(3 * W), st = buf(3 * 4112), sc = buf(3 * 16);
      std::vector<int32_t> per(3 * 16);
      int64_t FI[3] = {5, -7, 1}, NN[3] = {8995, 0, 4000};
      int32_t NR[3] = {16, 99, 2};                    // the idle item's ranges and parameters are not looked at
      int32_t RG[3 * 32], IP[18];
      float FP[12];
      for (int r = 0; r < 16; ++r) { RG[2 * r] = 500 * r; RG[2 * r + 1] = 500 * r + 200 + r; RG[32 + 2 * r] = 9; RG[33 + 2 * r] = 3; RG[64 + 2 * r] = 0; RG[65 + 2 * r] = 0; }
      RG[64] = 0; RG[65] = 10; RG[66] = 3990; RG[67] = 4000;           // a range at column 0 and one that ends with the item
      const int32_t gi[6] = {480, 60, 360, 240, 1200, 120};
      const float gf[4] = {1e-4f, 1e-12f, 1.f / 1200.f, 1.f / 121.f};
      for (int k = 0; k < 18; ++k) IP[k] = (k >= 6 && k < 12) ? -1 : gi[k % 6];
      for (int k = 0; k < 12; ++k) FP[k] = (k >= 4 && k < 8) ? NAN : gf[k % 4];
      std::vector<uint32_t> tab(48 * 3);
      int S = 3;
      int64_t pitch = 16, sp = 4112;
      auto scan = [&]() {
        return dmel_conceal_items(smp.data(), W, S, FI, NN, NR, RG, IP, FP, st.data(), sp, per.data(), sc.data(), pitch, tab.data(), nullptr);
      };
      CK(scan());
      auto refused = [&](const char* item, const char* what) {
        const int rc = scan();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL conceal_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = 65536; refused("65536 items", "more than 65535 items");
      S = 3; sp = 4111; refused("state pitch", "a state pitch below the row");
      sp = 4112; NN[2] = -1; refused("item 2", "a negative sample count");
      NN[2] = 4000; FI[0] = -1; refused("item 0", "a negative first column");
      FI[0] = 5; NR[2] = 17; refused("item 2", "17 ranges");
      NR[2] = 2; pitch = 15; refused("item 0", "more ranges than the output pitch");
      pitch = 16; RG[67] = 4001; refused("item 2", "a range behind the item's samples");
      RG[67] = 4000; RG[66] = 10; refused("item 2", "a range that touches the one before");
      RG[66] = 3990; RG[3] = RG[2]; refused("item 0", "an empty range");
      RG[3] = 701; RG[4] = 600; refused("item 0", "ranges that are not sorted");
      RG[4] = 1000; IP[0] = 484; refused("item 0", "a window that is no multiple of 8");
      IP[0] = 480; IP[13] = 7; refused("item 2", "Pmin below 8");
      IP[13] = 361; refused("item 2", "Pmin above Pmax");
      IP[13] = 60; IP[0] = 3744; refused("item 0", "a window and a period beyond the ring");
      IP[0] = 480; IP[15] = 2537; refused("item 2", "hold, fade and period beyond the ring");
      IP[15] = 240; IP[17] = 0; refused("item 2", "a recovery of 0");
      IP[17] = 120; FP[1] = 0.f; refused("item 0", "eps = 0");
      FP[1] = 1e-12f; FP[11] = 1.5f; refused("item 2", "rF above 1");
      FP[11] = 1.f / 121.f; FP[8] = INFINITY; refused("item 2", "a floor that is not finite");
      FP[8] = 0.f;                                  // a floor of 0 is allowed
      CK(scan());
      NN[0] = NN[2] = 0;                          // every item idle
      CK(scan());
    }
    {
      // the tone splice: tables of exactly R entries, a segment table of exactly 8 n_segs words, a table scratch of exactly
      // 6 R + 5 n_segs int64; its refusals read the host tables only
      auto out = buf(4096), speech = buf(2048), sine = buf(8000), ramps = buf(48);
      float* DST[4] = {out.data() + 1, out.data() + 101, out.data() + 101 + 360, nullptr};
      const float* SRC[4] = {speech.data() + 3, nullptr, speech.data() + 103, nullptr};
      int64_t NN[4] = {100, 360, 50, 0};
      int32_t SF[4] = {0, 0, 0, -7}, SC[4] = {0, 3, 0, 99};           // the idle part's segments are not looked at
      int32_t SEG[3 * 8] = {697, 1209, 0, 0, 100, 20, 24, 0, 941, 0, 0, 0, 96, 0, 48, 0, 350, 440, 0, 0, 100, 44, 0, -5};
      auto amp = [&](int k, int j, float a) { std::memcpy(SEG + 8 * k + 2 + j, &a, sizeof(float)); };
      amp(0, 0, 0.3f); amp(0, 1, 0.4f); amp(1, 0, 1.0f); amp(2, 0, 0.5f); amp(2, 1, 0.5f);
      SEG[8 + 7] = 0;                                                  // ramp tables of 24 and of 48 floats: [0, 24) and [0, 48)
      std::vector<int64_t> tab(6 * 4 + 5 * 3);
      int R = 4, n_segs = 3, rate = 8000;
      int64_t ramp_floats = 48;
      auto splice = [&]() { return dmel_tone_items(DST, SRC, NN, SF, SC, R, SEG, n_segs, sine.data(), rate, ramps.data(), ramp_floats, tab.data(), nullptr); };
      CK(splice());
      auto refused = [&](const char* part, const char* what) {
        const int rc = splice();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), part)) { std::printf("FAIL tone_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      R = 0; refused("0 parts", "no part");
      R = 65536; refused("65536 parts", "more than 65535 parts");
      R = 4; rate = 3999; refused("3999 Hz", "a rate below 4000 Hz");
      rate = 192001; refused("192001 Hz", "a rate above 192000 Hz");
      rate = 8000; NN[2] = -1; refused("part 2", "a negative sample count");
      NN[2] = 50; DST[0] = nullptr; refused("part 0", "a NULL destination");
      DST[0] = reinterpret_cast<float*>(reinterpret_cast<char*>(out.data()) + 2); refused("part 0", "a destination that is not 4-byte aligned");
      DST[0] = out.data() + 1; SC[1] = 4; refused("part 1", "a segment range behind the table");
      SC[1] = 0; refused("part 1", "a tone part without segments");
      SC[1] = 3; SF[1] = -1; refused("part 1", "a negative first segment");
      SF[1] = 0; NN[1] = 361; refused("part 1", "a part longer than its segments");
      NN[1] = 360; SEG[1] = 4000; refused("part 1", "a frequency of half the rate");
      SEG[1] = 1209; SEG[8 + 1] = 0; amp(1, 1, 0.1f); refused("part 1", "an amplitude with f = 0");
      amp(1, 1, 0.0f); amp(2, 1, 0.6f); refused("part 1", "amplitudes that sum above 1");
      amp(2, 1, NAN); refused("part 1", "an amplitude that is not a number");
      amp(2, 1, 0.5f); SEG[4] = 0; refused("part 1", "on = 0");
      SEG[4] = 100; SEG[8 + 5] = 1 << 24; refused("part 1", "off = 2^24");
      SEG[8 + 5] = 0; SEG[6] = 51; refused("part 1", "a ramp above half the tone");
      SEG[6] = 24; SEG[8 + 7] = 1; refused("part 1", "a ramp table that ends behind the arena");
      SEG[8 + 7] = 0; ramp_floats = 47; refused("part 1", "an arena shorter than a ramp table");
      ramp_floats = 48;
      // a second tone part on the same table: sharing a segment is fine where it begins at the same sample of both parts only
      DST[3] = out.data() + 600; NN[3] = 120; SF[3] = 0; SC[3] = 1;
      CK(splice());
      NN[3] = 96; SF[3] = 1; refused("part 3", "a segment that begins at sample 0 of this part and at sample 120 of an earlier one");
      DST[3] = nullptr; NN[3] = 0; SF[3] = -7; SC[3] = 99;
      NN[0] = NN[1] = NN[2] = 0; DST[0] = nullptr; SC[1] = 0;          // every part idle: pointers and segments are not looked at
      CK(splice());
    }
    {
      // reply shaping: tables of exactly S entries, a segment table of exactly 8 * 5 S words, a table scratch of exactly 64 S words; its
      // refusals read the host tables only.  The buffers are plain vectors: nothing here draws from the generator, so the weights of
      // the fingerprinted handles below stay what they were
      const int S0 = 3;
      std::vector<float> out(2048, 0.f), in(2048, 0.25f), ramps(48, 0.5f), pk(S0 * 8), gn(S0 * 8);
      std::vector<uint32_t> st((size_t)S0 * (16 + 127), 0u), tab(64 * S0);
      float* DST[S0] = {out.data() + 1, nullptr, out.data() + 1001};
      const float* SRC[S0] = {in.data() + 3, nullptr, in.data() + 1002};
      int64_t CAP[S0] = {192, -1, 300}, NN[S0] = {200, 0, 300}, HD[S0] = {70, -9, 0};
      int32_t FL[S0] = {2, 2, 1}, BL[S0] = {64, -5, 0}, SC[S0] = {2, 99, 0};       // the idle item's parameters are not looked at
      float FP[S0 * 5] = {0.98f, 0.1f, 1.f / 64.f, 1.f, 4.f, 0, 0, 0, 0, 0, 0.98f, 0.1f, 1.f / 120.f, 0.5f, 4.f};
      int32_t SEG[S0 * 8 * 5] = {0};
      auto seg = [&](int s, int k, int start, int ramp, int off, float g0, float g1) {
        int32_t* w = SEG + (8 * s + k) * 5;
        w[0] = start; w[1] = ramp; w[2] = off;
        std::memcpy(w + 3, &g0, sizeof(float)); std::memcpy(w + 4, &g1, sizeof(float));
      };
      seg(0, 0, -10, 48, 0, 1.f, 2.f); seg(0, 1, 100, 0, -3, 2.f, 0.f);
      int S = S0;
      int64_t ramp_floats = 48, pitch = 16 + 127, out_pitch = 8;
      auto shape = [&]() { return dmel_shape_items(DST, CAP, SRC, NN, HD, FL, BL, FP, SC, SEG, S, ramps.data(), ramp_floats, st.data(), pitch,
                                                   pk.data(), gn.data(), out_pitch, tab.data(), nullptr); };
      CK(shape());
      auto refused = [&](const char* item, const char* what) {
        const int rc = shape();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL shape_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = S0; CAP[0] = 191; refused("item 0", "a destination shorter than what the step hands out");
      CAP[0] = 192; HD[0] = 128; refused("item 0", "a hold of 2 N samples");
      HD[0] = 70; BL[0] = 31; refused("item 0", "a block of 31 samples");
      BL[0] = 64; pitch = 16 + 126; refused("item 0", "a state row shorter than header and hold");
      pitch = 16 + 127; out_pitch = 2; refused("item 0", "an output pitch below the blocks the step completes");
      out_pitch = 8; HD[2] = 1; refused("item 2", "held samples without the limiter");
      HD[2] = 0; CAP[2] = 299; refused("item 2", "a destination shorter than the samples of a step without the limiter");
      CAP[2] = 300; SRC[2] = nullptr; refused("item 2", "a NULL source");
      SRC[2] = in.data() + 1002; FP[10] = 0.f; refused("item 2", "a ceiling of 0");
      FP[10] = 0.98f; FP[13] = 4.5f; refused("item 2", "a base gain above max_gain");
      FP[13] = 0.5f; SC[0] = 9; refused("item 0", "nine segments");
      SC[0] = 2; seg(0, 1, -11, 0, 0, 2.f, 0.f); refused("item 0", "a start below the one before");
      seg(0, 1, 100, 0, -3, 2.f, 0.f); seg(0, 0, -10, 49, 0, 1.f, 2.f); refused("item 0", "a ramp table that ends behind the arena");
      seg(0, 0, -10, 48, 0, 1.f, NAN); refused("item 0", "a gain that is not a number");
      seg(0, 0, -10, 48, 0, 1.f, 2.f);
      CK(shape());
      NN[0] = NN[2] = 0; FL[2] = 0;               // every item idle
      CK(shape());
    }
    {
      // speaking rate: tables of exactly S entries, 5 S integers, 2 S float parameters, a request table of exactly 8 * 2 S words, a table
      // scratch of exactly 64 S words; its refusals read the host tables only.  Plain vectors, as above
      const int S0 = 3, Hh = 64, Dd = 8;
      std::vector<float> out(4096, 0.f), in(4096, 0.25f), wts(Hh, 0.5f), sc(S0 * 16);
      std::vector<int32_t> off(S0 * 16);
      std::vector<uint32_t> st((size_t)S0 * (16 + 2 * Hh + 2 * Dd), 0u), tab(64 * S0);
      float* DST[S0] = {out.data() + 1, nullptr, out.data() + 2001};
      const float* SRC[S0] = {in.data() + 3, nullptr, in.data() + 1002};
      int64_t CAP[S0] = {640, -1, 128}, NN[S0] = {640, 0, 100};
      // item 0 continues (K = 3, a_2 = 160, a_3 = 240, 400 fed, 100 held), item 1 is idle, item 2 is a whole short stream (final)
      int64_t IV[S0 * 5] = {3, 160, 240, 400, 100, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0};
      int32_t FL[S0] = {0, 0, 1}, HH[S0] = {Hh, -5, Hh}, DD[S0] = {Dd, -5, 0}, BP[S0] = {1250, 0, 2000}, RC[S0] = {2, 99, 0};
      int32_t WO[S0] = {0, -7, 0};
      float FP[S0 * 2] = {1e-6f, 1e-12f, 0, 0, 0.f, 1e-12f};
      int32_t RQ[S0 * 8 * 2] = {-50, 1500, 300, 700};
      int S = S0;
      int64_t wfloats = Hh, pitch = 16 + 2 * Hh + 2 * Dd, out_pitch = 16;
      auto pace = [&]() { return dmel_pace_items(DST, CAP, SRC, NN, IV, FL, HH, DD, FP, BP, RC, RQ, S, wts.data(), wfloats, WO, st.data(), pitch,
                                                 off.data(), sc.data(), out_pitch, tab.data(), nullptr); };
      CK(pace());
      auto refused = [&](const char* item, const char* what) {
        const int rc = pace();
        if (rc != DMEL_EINVAL || !std::strstr(dmel_last_error(), item)) { std::printf("FAIL pace_items accepted %s (%d: %s)\n", what, rc, dmel_last_error()); ++failures; }
      };
      S = 0; refused("0 items", "no item");
      S = S0; HH[0] = 56; refused("item 0", "a hop of 56 samples");
      HH[0] = 68; refused("item 0", "a hop that is no multiple of 8");
      HH[0] = Hh; DD[0] = 513; refused("item 0", "a search half-width of 513 samples");
      DD[0] = Dd; BP[0] = 499; refused("item 0", "a rate of 499 permille");
      BP[0] = 1250; RQ[3] = 2001; refused("item 0", "a request at 2001 permille");
      RQ[3] = 700; RQ[2] = -51; refused("item 0", "a request position below the one before");
      RQ[2] = 300; RC[0] = 9; refused("item 0", "nine requests");
      RC[0] = 2; IV[4] = 2 * Hh + 2 * Dd; refused("item 0", "a hold of 2 H + 2 D samples");
      IV[4] = 100; pitch = 16 + 2 * Hh + 2 * Dd - 1; refused("item 0", "a state row shorter than header and hold");
      pitch = 16 + 2 * Hh + 2 * Dd; CAP[0] = 63; refused("item 0", "a destination shorter than what the step hands out");
      CAP[0] = 640; out_pitch = 1; refused("item 0", "an output pitch below the frames the step completes");
      out_pitch = 16; IV[2] = 160 + 2 * Hh + 1; refused("item 0", "integers the rule cannot have made");
      IV[2] = 240; IV[12] = 5; refused("item 2", "a fresh slot with a_K = 5");
      IV[12] = 0; SRC[2] = nullptr; refused("item 2", "a NULL source");
      SRC[2] = in.data() + 1002; FP[4] = -1.f; refused("item 2", "a negative floor");
      FP[4] = 0.f; FP[1] = NAN; refused("item 0", "an eps that is not a number");
      FP[1] = 1e-12f; WO[2] = 1; refused("item 2", "a weight table that ends behind the arena");
      WO[2] = 0; FL[2] = 2; refused("item 2", "flags above 1");
      FL[2] = 1;
      CK(pace());
      NN[0] = NN[2] = 0; FL[2] = 0;               // every item idle
      CK(pace());
    }
    auto xs = buf(2 * 8 * 3000), ys = buf(2 * 8 * 3000), da = buf(8), db = buf(8);
    CK(dmel_aa_snake_f32(xs.data(), ys.data(), al.data(), be.data(), taps.data(), taps.data(), 1, 2, 8, 3000, nullptr));
    CK(dmel_aa_snake_backward_f32(xs.data(), ys.data(), xs.data(), al.data(), be.data(), da.data(), db.data(), taps.data(), taps.data(), 1, 2, 8, 3000, nullptr));
    {
      // the one-launch forms of the vocoder's head activations and tail: pointer tables, the alignment mask, the tap-count limit
      auto y1 = buf(2 * 8 * 3000), y2 = buf(2 * 8 * 3000), w = buf(8 * 257), yp = buf(2 * 3000);
      std::vector<int64_t> ln = {3000, 17};
      CK(dmel_aa_snake3_forward(xs.data(), ys.data(), y1.data() + 1, y2.data(), al.data(), be.data(), al.data(), nullptr, al.data(), be.data(),
                                taps.data(), taps.data(), 1, 2, 8, 3000, nullptr));
      CK(dmel_aa_snake3_forward_items(xs.data(), ys.data(), y1.data(), y2.data(), al.data(), be.data(), al.data(), nullptr, al.data(), be.data(),
                                      taps.data(), taps.data(), 0, 2, 8, 3000, ln.data(), nullptr));
      if (dmel_aa_snake3_forward(xs.data(), ys.data(), ys.data(), y2.data(), al.data(), be.data(), al.data(), nullptr, al.data(), be.data(),
                                 taps.data(), taps.data(), 1, 2, 8, 3000, nullptr) != DMEL_EINVAL) { std::printf("FAIL aa_snake3 accepted aliased outputs\n"); ++failures; }
      for (int K : {1, 7, 257})
        CK(dmel_snake_post_forward(xs.data(), al.data(), be.data(), taps.data(), taps.data(), 1, w.data(), 0.1f, 2, yp.data(), 2, 8, K, 3000, nullptr));
      CK(dmel_snake_post_forward_items(xs.data(), al.data(), nullptr, taps.data(), taps.data(), 1, w.data(), 0.f, 3, yp.data(), 2, 8, 7, 3000, ln.data(), nullptr));
      if (dmel_snake_post_forward(xs.data(), al.data(), be.data(), taps.data(), taps.data(), 1, w.data(), 0.f, 2, yp.data(), 2, 8, 259, 3000, nullptr) != DMEL_EINVAL ||
          !std::strstr(dmel_last_error(), "taps")) { std::printf("FAIL snake_post accepted 259 taps\n"); ++failures; }
    }
  }
  // drawn last, so that the handles above keep their weights: narrow encoder-like and conditioned stacks with every training image
  Fingerprinted fp;
  wavenet(10, 70, 70, 5, 4, 0, 4, 17, true);
  wavenet(48, 20, 48, 4, 4, 48, 2, 19, true);
  std::printf(failures ? "host ASan run: %d FAILURES\n" : "host ASan run: all entry points returned success, no sanitizer report\n", failures);
  return failures ? 1 : 0;
}
