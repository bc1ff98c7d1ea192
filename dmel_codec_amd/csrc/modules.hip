// Module-level orchestration: WaveNet, DownsampleFiniteScalarQuantize, BigVGAN.
// Host code only: consumes reference state-dict tensors, folds weight norm, re-tiles weights for the MFMA conv
// kernel and issues the kernel sequence of one forward on the caller's stream (no allocation, no sync).
#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>

#include "ops.h"

using namespace dmel;

namespace {

struct HostTensor {
  std::vector<float> v;
  std::vector<int64_t> shape;
  int64_t numel() const { return (int64_t)v.size(); }
};

struct TensorStore {
  std::map<std::string, HostTensor> t;
  int set(const char* key, const float* data, const int64_t* shape, int ndim) {
    DMEL_CHECK_ARG(key && data && shape && ndim >= 0 && ndim <= 4, "set_tensor: bad argument");
    HostTensor h;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { h.shape.push_back(shape[i]); n *= shape[i]; }
    h.v.assign(data, data + n);
    t[key] = std::move(h);
    return DMEL_OK;
  }
  const HostTensor* find(const std::string& k) const {
    auto it = t.find(k);
    return it == t.end() ? nullptr : &it->second;
  }
  // exact-shape lookup; sets the error and returns nullptr when missing or mis-shaped
  const HostTensor* need(const std::string& k, std::initializer_list<int64_t> shape) const {
    const HostTensor* h = find(k);
    if (!h) { set_error("missing state-dict tensor '%s'", k.c_str()); return nullptr; }
    if (h->shape != std::vector<int64_t>(shape)) {
      std::string got, want;
      for (auto s : h->shape) got += std::to_string(s) + ",";
      for (auto s : shape) want += std::to_string(s) + ",";
      set_error("tensor '%s' has shape (%s) but (%s) is required", k.c_str(), got.c_str(), want.c_str());
      return nullptr;
    }
    return h;
  }
  // w[i, ...] = g[i] * v[i, ...] / |v[i, ...]|: the sum of squares in double, the scale rounded to float before it multiplies
  static void fold_weight_norm(const HostTensor& v, const HostTensor& g, int64_t n0, std::vector<float>& out) {
    const int64_t inner = v.numel() / n0;
    out.resize(v.v.size());
    for (int64_t i = 0; i < n0; ++i) {
      double ss = 0;
      for (int64_t j = 0; j < inner; ++j) ss += (double)v.v[i * inner + j] * v.v[i * inner + j];
      const float scale = g.v[i] / (float)std::sqrt(ss);
      for (int64_t j = 0; j < inner; ++j) out[i * inner + j] = v.v[i * inner + j] * scale;
    }
  }
  // conv weight with optional old-style weight norm (weight_g, weight_v; norm over all dims but 0), torch._weight_norm
  bool conv_weight(const std::string& prefix, std::initializer_list<int64_t> shape, std::vector<float>& out) const {
    const int64_t n0 = *shape.begin();
    if (find(prefix + "weight")) {
      const HostTensor* w = need(prefix + "weight", shape);
      if (!w) return false;
      out = w->v;
      return true;
    }
    if (find(prefix + "parametrizations.weight.original1")) {      // torch.nn.utils.parametrizations.weight_norm (dim 0)
      const HostTensor* v1 = need(prefix + "parametrizations.weight.original1", shape);
      const HostTensor* g1 = find(prefix + "parametrizations.weight.original0");
      if (!v1 || !g1 || g1->numel() != n0) { set_error("missing or mis-shaped '%sparametrizations.weight.original0'", prefix.c_str()); return false; }
      fold_weight_norm(*v1, *g1, n0, out);
      return true;
    }
    const HostTensor* v = need(prefix + "weight_v", shape);
    if (!v) { set_error("missing state-dict tensor '%sweight' (or weight_g/weight_v)", prefix.c_str()); return false; }
    const HostTensor* g = find(prefix + "weight_g");
    if (!g || g->numel() != n0) { set_error("missing or mis-shaped '%sweight_g'", prefix.c_str()); return false; }
    fold_weight_norm(*v, *g, n0, out);
    return true;
  }
};

int upload_vec(DevBuf& d, const std::vector<float>& v) { return d.upload(v.data(), v.size() * sizeof(float)); }

ConvRun run_1seg(const float* x, int Cin, int64_t Tin, float* y, int Cout, int64_t Tout, int B) {
  ConvRun r;
  r.seg[0].x = x; r.seg[0].bstride = (int64_t)Cin * Tin; r.seg[0].cstride = Tin; r.seg[0].Tin = Tin;
  r.B = B; r.Tcols = Tout; r.y = y; r.y_bs = (int64_t)Cout * Tout; r.y_cs = Tout; r.Tout = Tout;
  return r;
}

// ---- base of the trainable handles (WaveNet, ConvNeXt, quantiser, discriminator) ---------------------------------------------------
// The state-dict store, the finalize / training flags and the table of where each parameter's gradient lies in the flat gradient buffer.
// The extern "C" entries forward to the train_* functions below with the module's name for the messages; a NULL handle is refused there.
struct TrainHandle {
  TensorStore ts;
  bool ready = false;
  bool train = false, train_ready = false;      // enable_training before finalize; train_ready: the training images are packed
  int train_precision = 0;                      // DMEL_PRECISION_BF16: bf16 training mode
  struct GradSlot { std::string key; int64_t offset, numel; };
  std::vector<GradSlot> slots;
  int64_t grad_floats = 0;
  void clear_slots() { slots.clear(); grad_floats = 0; }
  void add(const std::string& key, int64_t numel) { slots.push_back({key, grad_floats, numel}); grad_floats += numel; }
  int64_t offset_of(const std::string& key) const {
    for (const auto& s : slots)
      if (s.key == key) return s.offset;
    return -1;
  }
};
inline int train_set_tensor(TrainHandle* h, const char* key, const float* data, const int64_t* shape, int ndim) {
  DMEL_CHECK_ARG(h, "NULL handle");
  h->ready = false;
  return h->ts.set(key, data, shape, ndim);
}
inline int train_enable(TrainHandle* h, int on) {
  DMEL_CHECK_ARG(h, "NULL handle");
  h->train = on != 0;
  h->ready = false;          // takes effect at the next finalize (the host tensors are needed)
  h->train_ready = false;
  return DMEL_OK;
}
inline int train_set_precision(TrainHandle* h, const char* who, int precision) {
  DMEL_CHECK_ARG(h && (precision == DMEL_PRECISION_FP32 || precision == DMEL_PRECISION_BF16),
                 "%s_set_train_precision: DMEL_PRECISION_FP32 or DMEL_PRECISION_BF16", who);
  h->train_precision = precision;
  return DMEL_OK;
}
inline int64_t train_grad_floats(const TrainHandle* h) { return h && h->train_ready ? h->grad_floats : 0; }
// what: "a trained parameter of this WaveNet", ...
inline int train_grad_slot(const TrainHandle* h, const char* who, const char* what, const char* key, int64_t* offset, int64_t* numel) {
  DMEL_CHECK_ARG(h && key && offset && numel, "%s_grad_slot: NULL argument", who);
  if (!h->train_ready) { set_error("%s_grad_slot: training was not enabled before finalize", who); return DMEL_EMISSING; }
  for (const auto& s : h->slots)
    if (s.key == key) { *offset = s.offset; *numel = s.numel; return DMEL_OK; }
  set_error("%s_grad_slot: '%s' is not %s", who, key, what);
  return DMEL_EINVAL;
}

// ---- one description per weight image -----------------------------------------------------------------------------------------------
// A trainable convolution's packed image is described ONCE, as affine views (conv.h: RepackSeg / RepackSrc) over tensors that are named,
// not pointed to: by state-dict key, or as kFoldedWeight, "the weight-norm-folded weight of this layer".  finalize resolves the names to
// host pointers and packs with pack_conv through view_weight / view_bias; refresh resolves the same names to device pointers and hands
// the same views to launch_repack, whose kernel (train_ops.hip: repack_unit) evaluates them with the same addressing:
//   ro = (pC > 0 ? (sr % pC) * rs + (sr / pC) * ps : sr * rs) + (rev ? taps - 1 - tap : tap) * ts;   value = w[off + ro + ci * cs]
//   bias(sr) = b0[i] (+ b1[i]),  i = bias_mod ? sr % bias_mod : sr;   0 without a bias source
constexpr const char* kFoldedWeight = "#folded";
struct ImageSeg {
  std::string key;           // empty: the image has no such segment
  int64_t off = 0;           // base offset into the tensor, in floats
  int64_t rs = 0, cs = 0, ts = 0;
  int rev = 0;
  int64_t ps = 0;
  int pC = 0;
};
struct ImageSrc {
  ImageSeg seg[2];
  std::string b0, b1;
  int bias_mod = 0;
};
// the image and its description live together
struct WeightImage : PackedConv {
  ImageSrc src;
  bool described() const { return !src.seg[0].key.empty(); }
};

// rows x (Cin, taps) weight read as it lies: value(row, ci, tap) = w[(row * Cin + ci) * taps + tap]
inline ImageSeg seg_rows(const std::string& key, int Cin, int taps = 1) {
  ImageSeg s;
  s.key = key; s.rs = (int64_t)Cin * taps; s.cs = taps; s.ts = taps > 1 ? 1 : 0;
  return s;
}
// its transpose with the taps reversed, the backward-data image: value(row, cc, tap) = w[(cc * R + row) * taps + taps - 1 - tap]
inline ImageSeg seg_cols(const std::string& key, int R, int taps = 1) {
  ImageSeg s;
  s.key = key; s.rs = taps; s.cs = (int64_t)R * taps; s.ts = taps > 1 ? 1 : 0; s.rev = taps > 1;
  return s;
}

// names -> pointers; find(key) returns nullptr (error set) for a tensor that is not there
template <class Find> int resolve_image(const ImageSrc& src, Find&& find, RepackSrc& out) {
  for (int sg = 0; sg < 2; ++sg) {
    const ImageSeg& s = src.seg[sg];
    RepackSeg& o = out.seg[sg];
    if (s.key.empty()) continue;
    const float* w = find(s.key);
    if (!w) return DMEL_EMISSING;
    o.w = w + s.off; o.rs = s.rs; o.cs = s.cs; o.ts = s.ts; o.rev = s.rev; o.ps = s.ps; o.pC = s.pC;
  }
  for (int b = 0; b < 2; ++b) {
    const std::string& k = b ? src.b1 : src.b0;
    if (k.empty()) continue;
    const float* p = find(k);
    if (!p) return DMEL_EMISSING;
    (b ? out.b1 : out.b0) = p;
  }
  out.bias_mod = src.bias_mod;
  return DMEL_OK;
}

// the host evaluator: repack_unit's addressing (train_ops.hip), line for line
inline float view_weight(const RepackSeg& s, int taps, int sr, int ci, int tp) {
  const int t = s.rev ? taps - 1 - tp : tp;
  const int64_t ro = (s.pC > 0 ? (int64_t)(sr % s.pC) * s.rs + (int64_t)(sr / s.pC) * s.ps : (int64_t)sr * s.rs) + t * s.ts;
  return s.w[ro + (int64_t)ci * s.cs];
}
inline float view_bias(const RepackSrc& a, int sr) {
  float b = 0.f;
  const int bi = a.bias_mod > 0 ? sr % a.bias_mod : sr;
  if (a.b0) b = a.b0[bi];
  if (a.b1) b += a.b1[bi];
  return b;
}

// host route: record the description with the image and pack it from the store (and, for kFoldedWeight, from `folded`)
inline int pack_image(WeightImage& im, const PackDesc& d, ImageSrc src, const TensorStore& ts, const float* folded = nullptr) {
  im.src = std::move(src);
  RepackSrc v;
  DMEL_TRY(resolve_image(im.src, [&](const std::string& k) -> const float* {
    if (k == kFoldedWeight) return folded;
    const HostTensor* h = ts.find(k);
    if (!h) set_error("missing state-dict tensor '%s'", k.c_str());
    return h ? h->v.data() : nullptr;
  }, v));
  // the views are captured by value and the accessor is inlined into pack_conv's channel loop, as the per-image lambdas were
  const int taps[2] = {d.seg[0].taps, d.seg[1].taps};
  return pack_conv(im, d,
                   [v, taps](int sg, int sr, int ci, int tp) __attribute__((always_inline)) { return view_weight(v.seg[sg], taps[sg], sr, ci, tp); },
                   [v](int sr) { return view_bias(v, sr); });
}

// ---- the refresh skeleton -----------------------------------------------------------------------------------------------------------
// open() builds the key -> device pointer map; need() / add() resolve every tensor and image BEFORE the first copy or launch, so that a
// refused refresh leaves the handle as it was; run() makes the copies queued so far and sends the images added so far as ONE repack launch.
struct Refresh {
  const char* who;           // "wavenet_refresh", ...: the prefix of every message
  hipStream_t st;
  std::map<std::string, const float*> dev;
  std::vector<std::pair<PackedConv*, RepackSrc>> jobs;
  struct Copy { float* dst; const float* src; size_t count; };
  std::vector<Copy> copies;      // parameters that are used as they lie: plain device-to-device copies
  Refresh(const char* who_, void* stream) : who(who_), st((hipStream_t)stream) {}
  int open(int n, const char* const* keys, const float* const* device_tensors) {
    for (int i = 0; i < n; ++i) {
      DMEL_CHECK_ARG(keys[i] && device_tensors[i], "%s: NULL entry %d", who, i);
      dev[keys[i]] = device_tensors[i];
    }
    return DMEL_OK;
  }
  const float* find(const std::string& k) const {
    auto it = dev.find(k);
    if (it == dev.end()) { set_error("%s: tensor '%s' was not provided", who, k.c_str()); return nullptr; }
    return it->second;
  }
  int need(const std::string& k, const float** out) const { return (*out = find(k)) ? DMEL_OK : DMEL_EMISSING; }
  int add(WeightImage& im, const float* folded = nullptr) {
    if (!im.described()) return DMEL_OK;
    RepackSrc src;
    DMEL_TRY(resolve_image(im.src, [&](const std::string& k) { return k == kFoldedWeight ? folded : find(k); }, src));
    jobs.push_back({&im, src});
    return DMEL_OK;
  }
  int copy(float* dst, const std::string& key, size_t count) {
    const float* src;
    DMEL_TRY(need(key, &src));
    copies.push_back({dst, src, count});
    return DMEL_OK;
  }
  int run() {
    for (auto& c : copies) DMEL_HIP(hipMemcpyAsync(c.dst, c.src, c.count * sizeof(float), hipMemcpyDeviceToDevice, st));
    copies.clear();
    RepackBatch batch(st);
    for (auto& j : jobs) DMEL_TRY(launch_repack(*j.first, j.second, st));
    jobs.clear();
    return batch.flush();
  }
};

}  // namespace

// =====================================================================================================
// WaveNet                                               models/modules/wavenet.py:138-225
// =====================================================================================================
struct dmel_wavenet : TrainHandle {
  int Cin, Cout, C, L, cycle, Ccond;
  bool has_in = false, has_out = false;
  WeightImage in_proj, skip_proj, out_proj;
  std::vector<WeightImage> gate, resskip;
  int precision = 0;
  // training path (enable_training before finalize): unfused forward images that expose the gate pre-activations, and the
  // transposed images that turn every backward-data into a forward convolution
  struct TrainLayer { WeightImage pre_lin, out_lin, pre_dx, pre_dc, out_dz; int dil = 1; };
  std::vector<TrainLayer> tl;
  WeightImage in_dx, skip_dx, out_dx;
  WaveNetFused fused;          // whole-stack kernel for narrow unconditioned WaveNets on short items (the dMel encoder)
  // every image a refresh re-packs (those of absent projections carry no description and are passed over)
  template <class F> int each_image(F&& f) {
    DMEL_TRY(f(in_proj));
    for (int i = 0; i < L; ++i) { DMEL_TRY(f(gate[i])); DMEL_TRY(f(resskip[i])); }
    DMEL_TRY(f(skip_proj)); DMEL_TRY(f(out_proj));
    if (!train_ready) return DMEL_OK;
    DMEL_TRY(f(in_dx));
    for (auto& t : tl) { DMEL_TRY(f(t.pre_lin)); DMEL_TRY(f(t.out_lin)); DMEL_TRY(f(t.pre_dx)); DMEL_TRY(f(t.pre_dc)); DMEL_TRY(f(t.out_dz)); }
    DMEL_TRY(f(skip_dx));
    return f(out_dx);
  }
};


extern "C" int dmel_wavenet_create(dmel_wavenet** out, int input_channels, int output_channels, int residual_channels,
                                   int residual_layers, int dilation_cycle, int condition_channels) {
  DMEL_CHECK_ARG(out, "NULL out");
  DMEL_CHECK_ARG(residual_channels > 0 && residual_layers > 0 && dilation_cycle >= 0 && condition_channels >= 0,
                 "wavenet: bad configuration");
  auto* m = new dmel_wavenet();
  m->C = residual_channels;
  m->Cin = input_channels > 0 ? input_channels : residual_channels;
  m->Cout = output_channels > 0 ? output_channels : residual_channels;
  m->L = residual_layers; m->cycle = dilation_cycle; m->Ccond = condition_channels;
  m->has_in = m->Cin != m->C;     // wavenet.py:152-156
  m->has_out = m->Cout != m->C;   // wavenet.py:181-186
  *out = m;
  return DMEL_OK;
}
extern "C" void dmel_wavenet_destroy(dmel_wavenet* m) { delete m; }
extern "C" int dmel_wavenet_set_precision(dmel_wavenet* m, int precision) {
  DMEL_CHECK_ARG(m && valid_precision(precision), "wavenet_set_precision: not a DMEL_PRECISION_* value");
  m->precision = precision;
  return DMEL_OK;
}
extern "C" int dmel_wavenet_set_tensor(dmel_wavenet* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  return train_set_tensor(m, key, data, shape, ndim);
}

// 1x1 convolution `prefix` (Cout, Cin, 1) with its bias
static int pack_pointwise(WeightImage& im, const TensorStore& ts, const std::string& prefix, int Cout, int Cin) {
  const HostTensor* w = ts.need(prefix + "weight", {Cout, Cin, 1});
  const HostTensor* b = ts.need(prefix + "bias", {Cout});
  if (!w || !b) return DMEL_EMISSING;
  PackDesc d;
  d.mode = EPI_LINEAR; d.nseg = 1; d.C = Cout; d.seg[0].Cin = Cin;
  ImageSrc src;
  src.seg[0] = seg_rows(prefix + "weight", Cin); src.b0 = prefix + "bias";
  return pack_image(im, d, src, ts);
}

// transposed 1x1: y (rows = Cin of the forward conv) = W^T applied to a (Cout-channel) gradient; no bias
static int pack_pointwise_T(WeightImage& im, const TensorStore& ts, const std::string& key, int Cout, int Cin) {
  PackDesc d;
  d.mode = EPI_LINEAR; d.nseg = 1; d.C = Cin; d.seg[0].Cin = Cout;
  ImageSrc src;
  src.seg[0] = seg_cols(key, Cin);
  return pack_image(im, d, src, ts);
}

// checks the shapes of all tensors of residual layer `p` (dilated conv, output projection, condition projection) and describes the
// gate's two-segment source (dilated conv + condition projection, biases summed)
static int wavenet_layer_src(const dmel_wavenet* m, const std::string& p, ImageSrc& gate) {
  const int C = m->C, Cc = m->Ccond;
  const HostTensor* cw = m->ts.need(p + "conv_layer.conv.weight", {2 * C, C, 3});
  const HostTensor* cb = m->ts.need(p + "conv_layer.conv.bias", {2 * C});
  const HostTensor* ow = m->ts.need(p + "output_projection.conv.weight", {2 * C, C, 1});
  const HostTensor* ob = m->ts.need(p + "output_projection.conv.bias", {2 * C});
  if (!cw || !cb || !ow || !ob) return DMEL_EMISSING;
  gate = ImageSrc();
  gate.seg[0] = seg_rows(p + "conv_layer.conv.weight", C, 3); gate.b0 = p + "conv_layer.conv.bias";
  if (Cc) {
    const HostTensor* qw = m->ts.need(p + "condition_projection.conv.weight", {2 * C, Cc, 1});
    const HostTensor* qb = m->ts.need(p + "condition_projection.conv.bias", {2 * C});
    if (!qw || !qb) return DMEL_EMISSING;
    gate.seg[1] = seg_rows(p + "condition_projection.conv.weight", Cc); gate.b1 = p + "condition_projection.conv.bias";
  }
  return DMEL_OK;
}

static int wavenet_pack_training(dmel_wavenet* m) {
  const int C = m->C, Cc = m->Ccond;
  m->tl.clear();
  m->tl.resize(m->L);
  m->clear_slots();
  if (m->has_in) {
    if (!m->ts.need("input_projection.conv.weight", {C, m->Cin, 1})) return DMEL_EMISSING;
    DMEL_TRY(pack_pointwise_T(m->in_dx, m->ts, "input_projection.conv.weight", C, m->Cin));
    m->add("input_projection.conv.weight", (int64_t)C * m->Cin);
    m->add("input_projection.conv.bias", C);
  }
  for (int i = 0; i < m->L; ++i) {
    const std::string p = "residual_layers." + std::to_string(i) + ".";
    const int dil = m->cycle ? 1 << (i % m->cycle) : 1;
    dmel_wavenet::TrainLayer& t = m->tl[i];
    t.dil = dil;
    ImageSrc gate, out, dx;
    DMEL_TRY(wavenet_layer_src(m, p, gate));
    PackDesc d;      // pre-activation of the gate, rows in their natural order (wavenet.py:121-127)
    d.mode = EPI_LINEAR; d.C = 2 * C; d.nseg = Cc ? 2 : 1;
    d.seg[0].Cin = C; d.seg[0].taps = 3; d.seg[0].dil = dil; d.seg[0].pad_left = dil;
    d.seg[1].Cin = Cc;
    DMEL_TRY(pack_image(t.pre_lin, d, gate, m->ts));
    PackDesc e;
    e.mode = EPI_LINEAR; e.C = 2 * C; e.nseg = 1; e.seg[0].Cin = C;
    out.seg[0] = seg_rows(p + "output_projection.conv.weight", C); out.b0 = p + "output_projection.conv.bias";
    DMEL_TRY(pack_image(t.out_lin, e, out, m->ts));
    PackDesc g;      // d pre -> d x: transposed, tap-reversed dilated conv
    g.mode = EPI_LINEAR; g.C = C; g.nseg = 1;
    g.seg[0].Cin = 2 * C; g.seg[0].taps = 3; g.seg[0].dil = dil; g.seg[0].pad_left = dil;
    dx.seg[0] = seg_cols(p + "conv_layer.conv.weight", C, 3);
    DMEL_TRY(pack_image(t.pre_dx, g, dx, m->ts));
    if (Cc) DMEL_TRY(pack_pointwise_T(t.pre_dc, m->ts, p + "condition_projection.conv.weight", 2 * C, Cc));
    DMEL_TRY(pack_pointwise_T(t.out_dz, m->ts, p + "output_projection.conv.weight", 2 * C, C));
    m->add(p + "conv_layer.conv.weight", (int64_t)2 * C * C * 3);
    m->add(p + "conv_layer.conv.bias", 2 * C);
    if (Cc) {
      m->add(p + "condition_projection.conv.weight", (int64_t)2 * C * Cc);
      m->add(p + "condition_projection.conv.bias", 2 * C);
    }
    m->add(p + "output_projection.conv.weight", (int64_t)2 * C * C);
    m->add(p + "output_projection.conv.bias", 2 * C);
  }
  {
    if (!m->ts.need("skip_projection.conv.weight", {C, C, 1})) return DMEL_EMISSING;
    DMEL_TRY(pack_pointwise_T(m->skip_dx, m->ts, "skip_projection.conv.weight", C, C));
    m->add("skip_projection.conv.weight", (int64_t)C * C);
    m->add("skip_projection.conv.bias", C);
  }
  if (m->has_out) {
    if (!m->ts.need("output_projection.conv.weight", {m->Cout, C, 1})) return DMEL_EMISSING;
    DMEL_TRY(pack_pointwise_T(m->out_dx, m->ts, "output_projection.conv.weight", m->Cout, C));
    m->add("output_projection.conv.weight", (int64_t)m->Cout * C);
    m->add("output_projection.conv.bias", m->Cout);
  }
  m->train_ready = true;
  return DMEL_OK;
}

extern "C" int dmel_wavenet_set_train_precision(dmel_wavenet* m, int precision) { return train_set_precision(m, "wavenet", precision); }
extern "C" int dmel_wavenet_enable_training(dmel_wavenet* m, int on) { return train_enable(m, on); }

extern "C" int dmel_wavenet_finalize(dmel_wavenet* m) {
  DMEL_CHECK_ARG(m, "NULL handle");
  m->ready = m->train_ready = false;      // until every image is packed: a finalize that fails leaves a handle that refuses to run
  const int C = m->C;
  if (m->has_in) DMEL_TRY(pack_pointwise(m->in_proj, m->ts, "input_projection.conv.", C, m->Cin));
  m->gate.clear(); m->resskip.clear();
  m->gate.resize(m->L); m->resskip.resize(m->L);
  for (int i = 0; i < m->L; ++i) {
    const std::string p = "residual_layers." + std::to_string(i) + ".";
    const int dil = m->cycle ? 1 << (i % m->cycle) : 1;   // wavenet.py:169
    ImageSrc gate, out;
    DMEL_TRY(wavenet_layer_src(m, p, gate));
    PackDesc d;
    d.mode = EPI_GATE; d.C = C; d.nseg = m->Ccond ? 2 : 1;
    d.seg[0].Cin = C; d.seg[0].taps = 3; d.seg[0].dil = dil; d.seg[0].pad_left = dil;
    d.seg[1].Cin = m->Ccond;
    DMEL_TRY(pack_image(m->gate[i], d, gate, m->ts));
    PackDesc e;
    e.mode = EPI_RESSKIP; e.C = C; e.nseg = 1; e.seg[0].Cin = C;
    out.seg[0] = seg_rows(p + "output_projection.conv.weight", C); out.b0 = p + "output_projection.conv.bias";
    DMEL_TRY(pack_image(m->resskip[i], e, out, m->ts));
  }
  DMEL_TRY(pack_pointwise(m->skip_proj, m->ts, "skip_projection.conv.", C, C));
  if (m->has_out) DMEL_TRY(pack_pointwise(m->out_proj, m->ts, "output_projection.conv.", m->Cout, C));
  if (m->train) DMEL_TRY(wavenet_pack_training(m));
  // whole-stack kernel (wavenet_fused.hip): narrow, unconditioned, no output projection, dilations <= 8
  m->fused.ok = false;
  if (C > 32 && C <= 80 && !m->Ccond && !m->has_out && (!m->has_in || m->Cin <= 16) && (m->cycle == 0 || m->cycle <= 4)) {
    WaveNetFused& f = m->fused;
    f.Cin = m->Cin; f.C = C; f.L = m->L; f.cycle = m->cycle; f.has_in = m->has_in ? 1 : 0;
    f.skip_scale = (float)(1.0 / std::sqrt((double)m->L));
    f.in_w = m->has_in ? m->in_proj.w48.p : nullptr;
    f.in_b = m->has_in ? m->in_proj.bias.as<float>() : nullptr;
    f.skip_w = m->skip_proj.w48.p; f.skip_b = m->skip_proj.bias.as<float>();
    std::vector<const void*> tab((size_t)4 * m->L);
    for (int i = 0; i < m->L; ++i) {
      tab[i] = m->gate[i].w48.p;
      tab[m->L + i] = m->gate[i].bias.p;
      tab[2 * m->L + i] = m->resskip[i].w48.p;
      tab[3 * m->L + i] = m->resskip[i].bias.p;
    }
    DMEL_TRY(f.table.upload(tab.data(), tab.size() * sizeof(void*)));
    f.ok = true;
  }
  m->ts.t.clear();
  m->ready = true;
  return DMEL_OK;
}

// Folded batch: short items (1 s clips = 92 frames) leave the per-item tiling with 96-column tiles that do not divide the chip evenly
// (decoder of cfg 2: 35 row tiles x 32 items = 1120 wave tiles on 1024 SIMDs -> two rounds, the second 9 % full).  Laying the N items
// side by side on ONE time axis, each followed by max-dilation zero columns (the convolution's zero padding, shared by neighbours),
// turns every layer into a single long-row GEMM whose 128-column tiles pack the chip in one round (35 x 25 = 875 wave tiles).
struct FoldGeom {
  bool on = false;
  int P = 0;                 // item pitch = T + gap
  int64_t cols = 0, pitch = 0;
};
static FoldGeom wavenet_fold(const dmel_wavenet* m, int N, int64_t T) {
  // Opt-in (DMEL_WAVENET_FOLD=1, read per call so one process can A/B it): measured on the decoder of cfg 2 (profiles/r02_wavenet_fold.txt)
  // the folded launches are NOT faster with the current conv kernel -- 4.98 ms vs 4.12 ms per forward at the kernel's own tile choice,
  // 4.11 ms when forced onto the same 128 x 96 tile: a lone wave per SIMD runs the K loop at ~45 % of its MFMA time, so trading two
  // half-empty rounds for one full round of single waves gains nothing; what this shape needs is overlap inside a wave, not balance.
  const char* e = getenv("DMEL_WAVENET_FOLD");
  const int mode = e ? atoi(e) : 0;   // 0 off (default), 1 on
  const int max_t = 384;
  FoldGeom f;
  const int maxdil = m->cycle ? 1 << std::min(m->L - 1, m->cycle - 1) : 1;
  f.P = (int)T + maxdil;
  f.cols = (int64_t)N * f.P;
  f.pitch = (int64_t)align_up((size_t)f.cols, 32);
  f.on = N >= 2 && f.cols < ((int64_t)1 << 28) && mode == 1 && T <= max_t;
  return f;
}

struct WavePlan { float *xb, *zb, *sb, *tb, *cf, *xin, *yf; void *xp, *zp, *cp; size_t bytes; };
static WavePlan wavenet_plan(const dmel_wavenet* m, int N, int64_t T, void* ws) {
  Arena a(ws, (size_t)-1);
  WavePlan p{};
  const FoldGeom f = wavenet_fold(m, N, T);
  const size_t n = f.on ? (size_t)m->C * f.pitch : (size_t)N * m->C * T;
  p.xb = a.take<float>(n);
  p.zb = a.take<float>(n);
  p.sb = a.take<float>(n);
  p.tb = m->has_out ? a.take<float>(n) : nullptr;
  // pre-split operand planes of the fp16-split layered path (as many bytes as the fp32 tensors they shadow)
  p.xp = a.take<float>(n);
  p.zp = a.take<float>(n);
  p.cp = m->Ccond ? a.take<float>((size_t)N * m->Ccond * T) : nullptr;
  if (f.on) {
    p.cf = m->Ccond ? a.take<float>((size_t)m->Ccond * f.pitch) : nullptr;
    p.xin = m->has_in ? a.take<float>((size_t)m->Cin * f.pitch) : nullptr;
    p.yf = m->has_out ? a.take<float>((size_t)m->Cout * f.pitch) : nullptr;
  }
  p.bytes = align_up(a.off, 256);
  return p;
}

extern "C" size_t dmel_wavenet_workspace_bytes(const dmel_wavenet* m, int N, int64_t T) {
  if (!m || N <= 0 || T <= 0) return 0;
  return wavenet_plan(m, N, T, nullptr).bytes;
}

// one folded launch: input rows (Cin, pitch), output rows (Cout, pitch), all N items in one "batch item" of f.cols columns
static ConvRun run_folded(const FoldGeom& f, const float* x, float* y, int64_t T) {
  ConvRun r;
  r.seg[0].x = x; r.seg[0].bstride = 0; r.seg[0].cstride = f.pitch; r.seg[0].Tin = f.cols;
  r.B = 1; r.Tcols = f.cols; r.y = y; r.y_bs = 0; r.y_cs = f.pitch; r.Tout = f.cols;
  r.fold_pitch = f.P; r.fold_valid = (int)T;
  return r;
}

static int wavenet_forward_folded(const dmel_wavenet* m, const FoldGeom& f, const WavePlan& p, const float* x, const float* condition,
                                  float* y, int N, int64_t T, const int64_t* in_lengths, const int64_t* out_lengths, int div,
                                  hipStream_t st) {
  const int C = m->C;
  if (m->Ccond) DMEL_TRY(launch_fold(condition, p.cf, nullptr, 1, N, m->Ccond, T, f.P, f.pitch, st));
  if (m->has_in) {  // wavenet.py:205-207
    DMEL_TRY(launch_fold(x, p.xin, in_lengths, div, N, m->Cin, T, f.P, f.pitch, st));
    ConvRun r = run_folded(f, p.xin, p.xb, T);
    r.act = ACT_SILU; r.precision = m->precision;
    DMEL_TRY(launch_conv(m->in_proj, r, st));
  } else {
    DMEL_TRY(launch_fold(x, p.xb, in_lengths, div, N, C, T, f.P, f.pitch, st));
  }
  for (int i = 0; i < m->L; ++i) {  // wavenet.py:116-135
    ConvRun g = run_folded(f, p.xb, p.zb, T);
    if (m->Ccond) { g.seg[1].x = p.cf; g.seg[1].bstride = 0; g.seg[1].cstride = f.pitch; g.seg[1].Tin = f.cols; }
    g.precision = m->precision;
    DMEL_TRY(launch_conv(m->gate[i], g, st));
    ConvRun r = run_folded(f, p.zb, p.xb, T);
    r.skip = p.sb; r.skip_first = (i == 0);
    r.precision = m->precision;
    DMEL_TRY(launch_conv(m->resskip[i], r, st));
  }
  {  // wavenet.py:218-223
    float* proj = m->has_out ? p.tb : p.zb;
    ConvRun r = run_folded(f, p.sb, proj, T);
    r.seg[0].in_scale = (float)(1.0 / std::sqrt((double)m->L));
    if (m->has_out) r.act = ACT_SILU;
    r.precision = m->precision;
    DMEL_TRY(launch_conv(m->skip_proj, r, st));
    if (m->has_out) {
      ConvRun o = run_folded(f, p.tb, p.yf, T);
      o.precision = m->precision;
      DMEL_TRY(launch_conv(m->out_proj, o, st));
      proj = p.yf;
    }
    DMEL_TRY(launch_unfold(proj, y, out_lengths, div, N, m->Cout, T, f.P, f.pitch, st));
  }
  return DMEL_OK;
}

extern "C" int dmel_wavenet_forward(const dmel_wavenet* m, const float* x, const float* condition, float* y, int N, int64_t T,
                                    const int64_t* in_lengths, const int64_t* out_lengths, int group_repeat, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(m && x && y && workspace, "wavenet_forward: NULL argument");
  if (!m->ready) { set_error("wavenet_forward: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG((m->Ccond != 0) == (condition != nullptr), "wavenet_forward: condition tensor does not match the configuration");
  DMEL_CHECK_ARG(N > 0 && T > 0, "wavenet_forward: bad shape");
  // the lengths are indexed by n / group_repeat: a batch that is no multiple of it would read behind them
  DMEL_CHECK_ARG((!in_lengths && !out_lengths) || group_repeat <= 1 || N % group_repeat == 0,
                 "wavenet_forward: N = %d is no multiple of group_repeat = %d", N, group_repeat);
  const WavePlan p = wavenet_plan(m, N, T, workspace);
  float *xb = p.xb, *zb = p.zb, *sb = p.sb, *tb = p.tb;
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "wavenet_forward: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int C = m->C, div = group_repeat > 0 ? group_repeat : 1;
  {  // DMEL_WAVENET_FUSED=0 keeps the layered path (A/B); read per call
    const char* e = getenv("DMEL_WAVENET_FUSED");
    if (m->fused.ok && T <= 96 && m->precision == DMEL_PRECISION_FP32 && !(e && e[0] == '0') && !conv_fp32_mfma_forced())
      return launch_wavenet_fused(m->fused, x, y, in_lengths, out_lengths, div, N, T, st);
  }
  const FoldGeom fold = wavenet_fold(m, N, T);
  if (fold.on) return wavenet_forward_folded(m, fold, p, x, condition, y, N, T, in_lengths, out_lengths, div, st);

  if (m->has_in) {  // wavenet.py:205-207: 1x1 projection + SiLU
    ConvRun r = run_1seg(x, m->Cin, T, xb, C, T, N);
    r.seg[0].in_len = in_lengths; r.len_div = div; r.act = ACT_SILU;
    r.precision = m->precision;
    DMEL_TRY(launch_conv(m->in_proj, r, st));
  } else {
    DMEL_TRY(launch_masked_copy(x, xb, in_lengths, div, N, C, T, st));
  }
  // DMEL_WAVENET_PRESPLIT=1 (round-3 experiment, off by default): at the fp16-split precision every convolution of the stack reads its
  // input as PRE-SPLIT fp16 planes -- the condition is split once per forward instead of once per layer and row block (20 x 9 times for
  // the 560-channel decoder), the gate's output leaves its epilogue as planes only, the residual stream as fp32 + planes -- so that the
  // staging pass copies 16-byte units instead of converting.  Bit-identical (tests), and NOT faster: gate 114.9 vs 112.8 us, residual /
  // skip 46.5 vs 49.6 us per launch at 32 x 92 frames (rocprofv3, profiles/r03_conv_experiments.txt).  The operand conversion is not
  // what these kernels wait for either.
  const char* ps_env = getenv("DMEL_WAVENET_PRESPLIT");
  const bool presplit = m->precision == DMEL_PRECISION_FP32_F16X2 && C % 8 == 0 && (m->Ccond % 8) == 0 &&
                        (m->cycle ? 1 << std::min(m->L - 1, m->cycle - 1) : 1) <= 8 && ps_env && ps_env[0] == '1' && !conv_fp32_mfma_forced();
  const int64_t units = (int64_t)N * (C / 8) * T, cunits = (int64_t)N * (m->Ccond / 8) * T;
  if (presplit) {
    DMEL_TRY(launch_split_planes(xb, p.xp, units, nullptr, 1, N, C, T, st));
    if (m->Ccond) DMEL_TRY(launch_split_planes(condition, p.cp, cunits, nullptr, 1, N, m->Ccond, T, st));
  }
  for (int i = 0; i < m->L; ++i) {  // wavenet.py:116-135
    ConvRun g = run_1seg(xb, C, T, zb, C, T, N);
    if (m->Ccond) {
      g.seg[1].x = condition; g.seg[1].bstride = (int64_t)m->Ccond * T; g.seg[1].cstride = T; g.seg[1].Tin = T;
    }
    g.precision = m->precision;
    if (presplit) {
      g.seg[0].xp = p.xp; g.seg[0].xp_plane = units;
      if (m->Ccond) { g.seg[1].xp = p.cp; g.seg[1].xp_plane = cunits; }
      g.yp = p.zp; g.yp_plane = units; g.yp_only = 1;
    }
    DMEL_TRY(launch_conv(m->gate[i], g, st));
    ConvRun r = run_1seg(zb, C, T, xb, C, T, N);
    r.skip = sb; r.skip_first = (i == 0);
    r.precision = m->precision;
    if (presplit) {
      r.seg[0].xp = p.zp; r.seg[0].xp_plane = units;
      if (i + 1 < m->L) { r.yp = p.xp; r.yp_plane = units; }
    }
    DMEL_TRY(launch_conv(m->resskip[i], r, st));
  }
  {  // wavenet.py:218-223
    ConvRun r = run_1seg(sb, C, T, m->has_out ? tb : y, C, T, N);
    r.seg[0].in_scale = (float)(1.0 / std::sqrt((double)m->L));
    if (m->has_out) r.act = ACT_SILU;
    else { r.out_len = out_lengths; r.len_div = div; }
    r.precision = m->precision;
    DMEL_TRY(launch_conv(m->skip_proj, r, st));
    if (m->has_out) {
      ConvRun o = run_1seg(tb, C, T, y, m->Cout, T, N);
      o.out_len = out_lengths; o.len_div = div;
      o.precision = m->precision;
    DMEL_TRY(launch_conv(m->out_proj, o, st));
    }
  }
  return DMEL_OK;
}

// ---- incremental forward (include/dmel_hip.h: dmel_wavenet_stream_step) ----------------------------------------------------
// The frontier rules of one (prev, next) row; utt >= 0 names the utterance of a per-item table in the message.
static int stream_row_check(const dmel_wavenet* m, const int64_t* prev, const int64_t* next, int64_t cap, int64_t origin, int utt) {
  char who[48] = "";
  if (utt >= 0) std::snprintf(who, sizeof(who), "utterance %d: ", utt);
  const int L = m->L;
  const bool final_step = next[L] == next[0];
  for (int l = 0; l <= L; ++l) {
    DMEL_CHECK_ARG(prev[l] >= 0 && prev[l] <= next[l] && next[l] <= cap, "wavenet_stream_step: %slevel %d: need 0 <= prev <= next <= cap", who, l);
    if (l > 0) {
      const int dil = m->cycle ? 1 << ((l - 1) % m->cycle) : 1;
      DMEL_CHECK_ARG(final_step ? next[l] == next[0] : (next[l] == prev[l] || next[l] + dil <= next[l - 1]),
                     "wavenet_stream_step: %slevel %d runs ahead of its input (next %lld, input next %lld, dilation %d)", who, l,
                     (long long)next[l], (long long)next[l - 1], dil);
      DMEL_CHECK_ARG(prev[l] <= prev[l - 1], "wavenet_stream_step: %slevel %d is ahead of level %d", who, l, l - 1);
    }
  }
  if (origin > 0) {
    // column 0 is not the start of the sequence: a window that reaches in front of it would read zero padding where history belongs
    for (int l = 1; l <= L; ++l) {
      const int dil = m->cycle ? 1 << ((l - 1) % m->cycle) : 1;
      DMEL_CHECK_ARG(next[l] == prev[l] || prev[l] >= dil, "wavenet_stream_step: %slevel %d needs history in front of the buffer (origin %lld)",
                     who, l, (long long)origin);
    }
  }
  return DMEL_OK;
}

static int wavenet_stream_step_impl(const dmel_wavenet* m, const float* xraw, float* hist, float* skip, const float* cond, float* y,
                                    float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                    const int64_t* out_lengths, int group_repeat, int64_t origin, bool ex, void* stream);

extern "C" int dmel_wavenet_stream_step(const dmel_wavenet* m, float* hist, float* skip, const float* cond, float* y, float* scratch,
                                        int N, int64_t cap, const int64_t* prev, const int64_t* next, void* stream) {
  return wavenet_stream_step_impl(m, nullptr, hist, skip, cond, y, scratch, N, cap, prev, next, nullptr, 1, 0, false, stream);
}

extern "C" int dmel_wavenet_stream_step_ex(const dmel_wavenet* m, const float* x, float* hist, float* skip, const float* cond, float* y,
                                           float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                           const int64_t* out_lengths, int group_repeat, int64_t origin, void* stream) {
  return wavenet_stream_step_impl(m, x, hist, skip, cond, y, scratch, N, cap, prev, next, out_lengths, group_repeat, origin, true, stream);
}

// per-utterance frontiers (include/dmel_hip.h): every row checked, then the one-launch kernel over all items -- or nothing
extern "C" int dmel_wavenet_stream_step_items(const dmel_wavenet* m, const float* x, float* hist, float* skip, const float* cond, float* y,
                                              float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                              const int64_t* out_lengths, int group_repeat, const int64_t* origin, void* stream) {
  DMEL_CHECK_ARG(m && hist && skip && y && scratch && prev && next && origin, "wavenet_stream_step_items: NULL argument");
  if (!m->ready) { set_error("wavenet_stream_step_items: handle not finalized"); return DMEL_EMISSING; }
  if (m->Ccond || cond || !m->fused.ok || m->L > kStreamMaxL || m->precision != DMEL_PRECISION_FP32 || conv_fp32_mfma_forced()) {
    set_error("wavenet_stream_step_items: only the stacks of the one-launch kernel are taken (residual channels in (32, 80], no condition, no "
              "output projection, dilations <= 8, DMEL_PRECISION_FP32); there is no layered per-item step");
    return DMEL_EUNSUPPORTED;
  }
  DMEL_CHECK_ARG(m->has_in == (x != nullptr), "wavenet_stream_step_items: the raw input is given exactly when the model has an input projection");
  const int div = group_repeat > 0 ? group_repeat : 1;
  DMEL_CHECK_ARG(N > 0 && cap > 0 && N % div == 0, "wavenet_stream_step_items: bad shape / group_repeat");
  const int R = N / div, L1 = m->L + 1;
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(origin[r] >= 0, "wavenet_stream_step_items: utterance %d: negative origin", r);
    DMEL_TRY(stream_row_check(m, prev + (size_t)r * L1, next + (size_t)r * L1, cap, origin[r], r));
  }
  // the table lies behind dmel_wavenet_stream_step_ex's scratch: N * 2 C * cap floats, N int64
  int32_t* tab = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + (size_t)2 * N * m->C * cap * sizeof(float) + (size_t)N * sizeof(int64_t));
  return launch_wavenet_stream_items(m->fused, x, hist, skip, y, out_lengths, div, N, cap, prev, next, tab, (hipStream_t)stream);
}

// Per-utterance frontiers through the LAYERED step (include/dmel_hip.h): wavenet_stream_step_impl's launches below, each over all N items
// with per-item column windows (ConvRun::win) read from ONE device table of the rows -- prev[0..L] | next[0..L] per utterance, uploaded
// once -- so every launch only names the level it works on.  Any stack the layered lockstep step serves.
extern "C" int dmel_wavenet_stream_step_items_layered(const dmel_wavenet* m, const float* x, float* hist, float* skip, const float* cond,
                                                      float* y, float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                                      const int64_t* out_lengths, int group_repeat, const int64_t* origin, void* stream) {
  DMEL_CHECK_ARG(m && hist && skip && y && scratch && prev && next && origin, "wavenet_stream_step_items_layered: NULL argument");
  if (!m->ready) { set_error("wavenet_stream_step_items_layered: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG((m->Ccond != 0) == (cond != nullptr), "wavenet_stream_step_items_layered: condition tensor does not match the configuration");
  DMEL_CHECK_ARG(m->has_in == (x != nullptr), "wavenet_stream_step_items_layered: the raw input is given exactly when the model has an input projection");
  const int div = group_repeat > 0 ? group_repeat : 1;
  DMEL_CHECK_ARG(N > 0 && N <= 65535 && cap > 0 && cap < ((int64_t)1 << 30) && N % div == 0, "wavenet_stream_step_items_layered: bad shape / group_repeat");
  if (conv_fp32_mfma_forced() || m->precision == DMEL_PRECISION_FP32_MFMA || m->precision == DMEL_PRECISION_BF16 ||
      train_precision_override() == DMEL_PRECISION_BF16) {
    set_error("wavenet_stream_step_items_layered: per-item column windows are built into the split kernels only (DMEL_PRECISION_FP32 / "
              "FP32_BF16X3 / FP32_F16X2); a forced native fp32 MFMA and the bf16-operand mode are not served");
    return DMEL_EUNSUPPORTED;
  }
  const int C = m->C, L = m->L, L1 = L + 1, R = N / div, RI = kStreamRowInts(L);
  for (int r = 0; r < R; ++r) {
    DMEL_CHECK_ARG(origin[r] >= 0, "wavenet_stream_step_items_layered: utterance %d: negative origin", r);
    DMEL_TRY(stream_row_check(m, prev + (size_t)r * L1, next + (size_t)r * L1, cap, origin[r], r));
  }
  // the table: prev[0..L] | next[0..L] | idle flag per utterance; per level the largest window, the columns of all items and the active items
  std::vector<int32_t> rows((size_t)R * RI);
  std::vector<int64_t> maxc(L1, 0), sumc(L1, 0);
  std::vector<int> act(L1, 0);
  for (int r = 0; r < R; ++r) {
    bool idle = true;
    for (int l = 0; l < L1; ++l) {
      const int64_t p = prev[(size_t)r * L1 + l], n = next[(size_t)r * L1 + l];
      rows[(size_t)r * RI + l] = (int32_t)p;
      rows[(size_t)r * RI + L1 + l] = (int32_t)n;
      maxc[l] = std::max(maxc[l], n - p);
      sumc[l] += div * (n - p);
      if (n > p) { act[l] += div; idle = false; }
    }
    rows[(size_t)r * RI + 2 * L1] = idle ? -1 : 0;
  }
  hipStream_t st = (hipStream_t)stream;
  // behind dmel_wavenet_stream_step_ex's scratch (N * 2 C * cap floats, N int64), as dmel_wavenet_stream_step_items places its table
  const int64_t bs = (int64_t)C * cap, lvl = (int64_t)N * bs;
  int64_t* rel = reinterpret_cast<int64_t*>(scratch + 2 * lvl);
  int32_t* tab = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + (size_t)2 * lvl * sizeof(float) + (size_t)N * sizeof(int64_t));
  bool any = false;
  for (int l = 0; l < L1; ++l) any = any || maxc[l] > 0;
  if (!any) return DMEL_OK;                     // every row idle: nothing to do
  DMEL_TRY(launch_table_put(rows.data(), rows.size() * sizeof(int32_t), tab, st));
  float* zb = scratch;                          // gate output of the block being computed, (N, C, cap)
  // new columns of level `lev` from an input whose valid length is next[vlev]: the windows of wavenet_stream_step_impl's sub(), per item
  auto sub = [&](const float* xin, int Cin, int vlev, int lev, float* out, int Cout) {
    ConvRun r;
    r.seg[0].x = xin; r.seg[0].bstride = (int64_t)Cin * cap; r.seg[0].cstride = cap;
    r.B = N; r.Tcols = maxc[lev]; r.y = out; r.y_bs = (int64_t)Cout * cap; r.y_cs = cap; r.Tout = maxc[lev];
    r.len_div = div;
    r.win = tab; r.win_stride = RI; r.win_shift = lev; r.win_end = L1 + lev; r.win_valid[0] = L1 + vlev;
    r.win_cols_total = sumc[lev]; r.win_active = act[lev];
    r.precision = m->precision;
    return r;
  };
  if (m->has_in && maxc[0] > 0) {  // wavenet.py:205-207 on the new columns of level 0
    ConvRun r = sub(x, m->Cin, 0, 0, hist, C);
    r.act = ACT_SILU;
    DMEL_TRY(launch_conv(m->in_proj, r, st));
  }
  for (int i = 0; i < L; ++i) {  // wavenet.py:116-135 on the new columns of block i + 1
    if (maxc[i + 1] <= 0) continue;
    const float* xin = hist + (int64_t)i * lvl;
    float* xout = hist + (int64_t)(i + 1) * lvl;
    ConvRun g = sub(xin, C, i, i + 1, zb, C);
    if (m->Ccond) {
      g.seg[1].x = cond; g.seg[1].bstride = (int64_t)m->Ccond * cap; g.seg[1].cstride = cap; g.win_valid[1] = L1 + 0;
    }
    DMEL_TRY(launch_conv(m->gate[i], g, st));
    // block i's input survives as history: its new columns are copied into block i + 1's rows and updated there (see the lockstep step)
    DMEL_TRY(launch_copy_windows(xin, xout, N, C, cap, tab, RI, i + 1, L1 + i + 1, div, maxc[i + 1], sumc[i + 1], st));
    ConvRun r = sub(zb, C, i + 1, i + 1, xout, C);
    r.skip = skip; r.skip_first = (i == 0);
    DMEL_TRY(launch_conv(m->resskip[i], r, st));
  }
  if (maxc[L] > 0) {  // wavenet.py:218-223 on the columns whose skip sum is complete
    float* tb = scratch + lvl;                  // second half of the scratch
    ConvRun r = sub(skip, C, L, L, m->has_out ? tb : y, C);
    r.seg[0].in_scale = (float)(1.0 / std::sqrt((double)m->L));
    // the output mask in the store: an item's columns start at its prev[L], so its length is taken relative to that
    if (out_lengths) DMEL_TRY(launch_shift_lengths_items(out_lengths, tab, RI, L, rel, R, st));
    if (m->has_out) r.act = ACT_SILU;
    else r.out_len = out_lengths ? rel : nullptr;
    DMEL_TRY(launch_conv(m->skip_proj, r, st));
    if (m->has_out) {
      ConvRun o = sub(tb, C, L, L, y, m->Cout);
      o.out_len = out_lengths ? rel : nullptr;
      DMEL_TRY(launch_conv(m->out_proj, o, st));
    }
  }
  return DMEL_OK;
}

static int wavenet_stream_step_impl(const dmel_wavenet* m, const float* xraw, float* hist, float* skip, const float* cond, float* y,
                                    float* scratch, int N, int64_t cap, const int64_t* prev, const int64_t* next,
                                    const int64_t* out_lengths, int group_repeat, int64_t origin, bool ex, void* stream) {
  DMEL_CHECK_ARG(m && hist && skip && y && scratch && prev && next, "wavenet_stream_step: NULL argument");
  if (!m->ready) { set_error("wavenet_stream_step: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG((m->Ccond != 0) == (cond != nullptr), "wavenet_stream_step: condition tensor does not match the configuration");
  if (!ex && m->has_in) { set_error("wavenet_stream_step: models with an input projection are not supported (the decoder has none)"); return DMEL_EUNSUPPORTED; }
  DMEL_CHECK_ARG(m->has_in == (xraw != nullptr), "wavenet_stream_step: the raw input is given exactly when the model has an input projection");
  DMEL_CHECK_ARG(N > 0 && cap > 0, "wavenet_stream_step: bad shape");
  const int div = group_repeat > 0 ? group_repeat : 1;
  DMEL_CHECK_ARG(origin >= 0 && (!out_lengths || N % div == 0), "wavenet_stream_step: bad origin / group_repeat");
  const int C = m->C, L = m->L;
  DMEL_TRY(stream_row_check(m, prev, next, cap, origin, -1));
  hipStream_t st = (hipStream_t)stream;
  if (ex) {  // DMEL_WAVENET_STREAM_FUSED=0 keeps the layered step (A/B); read per call
    const char* e = getenv("DMEL_WAVENET_STREAM_FUSED");
    if (m->fused.ok && L <= kStreamMaxL && m->precision == DMEL_PRECISION_FP32 && !(e && e[0] == '0') && !conv_fp32_mfma_forced())
      return launch_wavenet_stream(m->fused, xraw, hist, skip, y, out_lengths, div, N, cap, prev, next, st);
  }
  const int64_t bs = (int64_t)C * cap, lvl = (int64_t)N * bs;
  float* zb = scratch;                        // gate output of the block being computed, (N, C, cap)
  auto sub = [&](const float* x, int Cin, int64_t valid, int64_t p, float* out, int Cout, int64_t cols) {
    ConvRun r;
    r.seg[0].x = x; r.seg[0].bstride = (int64_t)Cin * cap; r.seg[0].cstride = cap; r.seg[0].Tin = valid; r.seg[0].tshift = p;
    r.B = N; r.Tcols = cols; r.y = out + p; r.y_bs = (int64_t)Cout * cap; r.y_cs = cap; r.Tout = cols;
    r.precision = m->precision;
    return r;
  };
  if (m->has_in && next[0] > prev[0]) {  // wavenet.py:205-207 on the new columns of level 0
    ConvRun r = sub(xraw, m->Cin, next[0], prev[0], hist, C, next[0] - prev[0]);
    r.act = ACT_SILU;
    DMEL_TRY(launch_conv(m->in_proj, r, st));
  }
  for (int i = 0; i < L; ++i) {  // wavenet.py:116-135 on the new columns of block i + 1
    const int64_t p = prev[i + 1], cols = next[i + 1] - p;
    if (cols <= 0) continue;
    const float* xin = hist + (int64_t)i * lvl;
    float* xout = hist + (int64_t)(i + 1) * lvl;
    ConvRun g = sub(xin, C, next[i], p, zb, C, cols);
    if (m->Ccond) {
      g.seg[1].x = cond; g.seg[1].bstride = (int64_t)m->Ccond * cap; g.seg[1].cstride = cap; g.seg[1].Tin = next[0]; g.seg[1].tshift = p;
    }
    DMEL_TRY(launch_conv(m->gate[i], g, st));
    // the residual update is in place in the whole-sequence kernel ((x + r) / sqrt2 over x): here block i's input must survive as
    // history, so its new columns are first copied into block i + 1's rows and updated there
    DMEL_HIP(hipMemcpy2DAsync(xout + p, (size_t)cap * sizeof(float), xin + p, (size_t)cap * sizeof(float), (size_t)cols * sizeof(float),
                              (size_t)N * C, hipMemcpyDeviceToDevice, st));
    ConvRun r = sub(zb, C, next[i + 1], p, xout, C, cols);
    r.skip = skip + p; r.skip_first = (i == 0);
    DMEL_TRY(launch_conv(m->resskip[i], r, st));
  }
  {  // wavenet.py:218-223 on the columns whose skip sum is complete
    const int64_t p = prev[L], cols = next[L] - p;
    if (cols > 0) {
      float* tb = scratch + (int64_t)N * bs;    // second half of the scratch
      ConvRun r = sub(skip, C, next[L], p, m->has_out ? tb : y, C, cols);
      r.seg[0].in_scale = (float)(1.0 / std::sqrt((double)m->L));
      // the output mask of the whole-sequence call, in the store: the launch's columns start at p, so its lengths are taken relative to p
      int64_t* rel = nullptr;
      if (out_lengths) {
        rel = reinterpret_cast<int64_t*>(scratch + 2 * (int64_t)N * bs);
        DMEL_TRY(launch_shift_lengths(out_lengths, p, rel, N / div, st));
      }
      if (m->has_out) r.act = ACT_SILU;
      else { r.out_len = rel; r.len_div = div; }
      DMEL_TRY(launch_conv(m->skip_proj, r, st));
      if (m->has_out) {
        ConvRun o = sub(tb, C, next[L], p, y, m->Cout, cols);
        o.out_len = rel; o.len_div = div;
        DMEL_TRY(launch_conv(m->out_proj, o, st));
      }
    }
  }
  return DMEL_OK;
}

// ---- WaveNet training path --------------------------------------------------------------------------------------
// forward_train computes exactly wavenet.py:204-225 but unfused, keeping what backward needs (every block's input, gate
// pre-activation and gated output; the SiLU inputs); backward is reverse-mode differentiation of that graph -- what
// `manual_backward(loss)` (codec_lit_modules.py:236,315) does through autograd -- built from: backward-data = the forward
// conv kernel on transposed weights, backward-weight = conv_wgrad_kernel, and the elementwise kernels of train_ops.hip.
namespace {
struct TrainPlan {
  float *X, *PRE, *Z, *U, *XS, *P, *Q, *SK, *O;          // saved by forward (X: L+1 slabs, PRE: L x 2n, Z: L slabs)
  float *GXa, *GXb, *GS, *GO, *GXS, *DZ, *DPRE, *DP, *DQ;   // backward temporaries
  size_t n, bytes;
};
TrainPlan train_plan(const dmel_wavenet* m, int N, int64_t T, void* ws) {
  TrainPlan p{};
  Arena a(ws, (size_t)-1);
  const size_t n = (size_t)N * m->C * T;
  p.n = n;
  p.X = a.take<float>(n * (m->L + 1));
  p.PRE = a.take<float>(2 * n * m->L);
  p.Z = a.take<float>(n * m->L);
  p.U = m->has_in ? a.take<float>(n) : nullptr;
  p.XS = a.take<float>(n);
  p.P = a.take<float>(n);
  p.Q = m->has_out ? a.take<float>(n) : nullptr;
  p.SK = a.take<float>(n);
  p.O = a.take<float>(2 * n);
  p.GXa = a.take<float>(n);
  p.GXb = a.take<float>(n);
  p.GS = a.take<float>(n);
  p.GO = a.take<float>(2 * n);
  p.GXS = a.take<float>(n);
  p.DZ = a.take<float>(n);
  p.DPRE = a.take<float>(2 * n);
  p.DP = a.take<float>(n);
  p.DQ = m->has_out ? a.take<float>(n) : nullptr;
  p.bytes = align_up(a.off, 256);
  return p;
}
int train_precision(const dmel_wavenet* m) { return exact_precision(m->precision); }
}  // namespace

extern "C" int dmel_wavenet_refresh(dmel_wavenet* m, int n, const char* const* keys, const float* const* device_tensors,
                                    void* stream) {
  DMEL_CHECK_ARG(m && keys && device_tensors && n > 0, "wavenet_refresh: bad argument");
  if (!m->ready) { set_error("wavenet_refresh: handle not finalized"); return DMEL_EMISSING; }
  Refresh r("wavenet_refresh", stream);
  DMEL_TRY(r.open(n, keys, device_tensors));
  DMEL_TRY(m->each_image([&](WeightImage& im) { return r.add(im); }));
  return r.run();      // all convolutions of the network in one launch
}

extern "C" size_t dmel_wavenet_train_workspace_bytes(const dmel_wavenet* m, int N, int64_t T) {
  if (!m || N <= 0 || T <= 0) return 0;
  return train_plan(m, N, T, nullptr).bytes;
}
extern "C" int64_t dmel_wavenet_grad_floats(const dmel_wavenet* m) { return train_grad_floats(m); }
extern "C" int dmel_wavenet_grad_slot(const dmel_wavenet* m, const char* key, int64_t* offset, int64_t* numel) {
  return train_grad_slot(m, "wavenet", "a trained parameter of this WaveNet", key, offset, numel);
}

extern "C" int dmel_wavenet_forward_train(const dmel_wavenet* m, const float* x, const float* condition, float* y, int N, int64_t T,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(m ? m->train_precision : 0);
  DMEL_CHECK_ARG(m && x && y && workspace, "wavenet_forward_train: NULL argument");
  if (!m->ready || !m->train_ready) { set_error("wavenet_forward_train: enable_training + finalize first"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG((m->Ccond != 0) == (condition != nullptr), "wavenet_forward_train: condition tensor does not match the configuration");
  DMEL_CHECK_ARG(N > 0 && T > 0, "wavenet_forward_train: bad shape");
  const TrainPlan p = train_plan(m, N, T, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "wavenet_forward_train: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  // the forward of a CONDITIONED WaveNet (the decoder: nothing discrete downstream) runs on the three-product fp16 split like its inference
  // forward; an unconditioned one (the encoder: its output is quantised) and every backward pass keep the six-product split
  const int C = m->C, prec = (train_precision(m) == DMEL_PRECISION_FP32 && m->Ccond > 0) ? DMEL_PRECISION_FP32_F16X2 : train_precision(m);
  const size_t n = p.n;
  if (m->has_in) {  // wavenet.py:205-207
    ConvRun r = run_1seg(x, m->Cin, T, p.U, C, T, N);
    r.precision = prec;
    DMEL_TRY(launch_conv(m->in_proj, r, st));
    DMEL_TRY(launch_silu_fwd(p.U, p.X, (int64_t)n, st));
  } else {
    DMEL_HIP(hipMemcpyAsync(p.X, x, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  for (int i = 0; i < m->L; ++i) {  // wavenet.py:116-135
    const float* xi = p.X + (size_t)i * n;
    float* pre = p.PRE + (size_t)i * 2 * n;
    float* z = p.Z + (size_t)i * n;
    ConvRun g = run_1seg(xi, C, T, pre, 2 * C, T, N);
    if (m->Ccond) { g.seg[1].x = condition; g.seg[1].bstride = (int64_t)m->Ccond * T; g.seg[1].cstride = T; g.seg[1].Tin = T; }
    g.precision = prec;
    DMEL_TRY(launch_conv(m->tl[i].pre_lin, g, st));
    DMEL_TRY(launch_gate_fwd(pre, z, N, C, T, st));
    ConvRun o = run_1seg(z, C, T, p.O, 2 * C, T, N);
    o.precision = prec;
    DMEL_TRY(launch_conv(m->tl[i].out_lin, o, st));
    DMEL_TRY(launch_resskip_fwd(xi, p.O, p.X + (size_t)(i + 1) * n, p.SK, i == 0, N, C, T, st));
  }
  DMEL_TRY(launch_scale(p.SK, p.XS, (float)(1.0 / std::sqrt((double)m->L)), (int64_t)n, st));   // wavenet.py:218
  {
    ConvRun r = run_1seg(p.XS, C, T, m->has_out ? p.P : y, C, T, N);
    r.precision = prec;
    DMEL_TRY(launch_conv(m->skip_proj, r, st));
  }
  if (m->has_out) {  // wavenet.py:221-223
    DMEL_TRY(launch_silu_fwd(p.P, p.Q, (int64_t)n, st));
    ConvRun o = run_1seg(p.Q, C, T, y, m->Cout, T, N);
    o.precision = prec;
    DMEL_TRY(launch_conv(m->out_proj, o, st));
  }
  return DMEL_OK;
}

extern "C" int dmel_wavenet_backward(const dmel_wavenet* m, const float* x, const float* condition, const float* dy, float* dx,
                                     float* dcondition, float* grads, int N, int64_t T, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return dmel_wavenet_backward_hooked(m, x, condition, dy, dx, dcondition, grads, N, T, workspace, workspace_bytes, stream, nullptr, nullptr);
}

extern "C" int dmel_wavenet_backward_hooked(const dmel_wavenet* m, const float* x, const float* condition, const float* dy, float* dx,
                                            float* dcondition, float* grads, int N, int64_t T, void* workspace,
                                            size_t workspace_bytes, void* stream, dmel_grad_ready_fn on_ready, void* user) {
  TrainPrecisionScope train_scope(m ? m->train_precision : 0);
  DMEL_CHECK_ARG(m && x && dy && grads && workspace, "wavenet_backward: NULL argument");
  if (!m->ready || !m->train_ready) { set_error("wavenet_backward: enable_training + finalize first"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG((m->Ccond != 0) == (condition != nullptr), "wavenet_backward: condition tensor does not match the configuration");
  DMEL_CHECK_ARG(N > 0 && T > 0, "wavenet_backward: bad shape");
  const TrainPlan p = train_plan(m, N, T, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "wavenet_backward: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int C = m->C, Cc = m->Ccond, prec = train_precision(m);
  const size_t n = p.n;
  ClearedRange cleared(grads, (size_t)m->grad_floats * sizeof(float), st);      // one memset for the ~120 gradient tensors of the network
  DMEL_TRY(cleared.error());
  auto G = [&](const std::string& key) -> float* {
    const int64_t o = m->offset_of(key);
    return o < 0 ? nullptr : grads + o;
  };
  // contiguous region of the flat gradient buffer that belongs to the slots whose key starts with `prefix` (slots are laid out
  // input_projection | residual_layers.0 | ... | residual_layers.L-1 | skip_projection | output_projection)
  auto ready = [&](const std::string& prefix, const std::string& prefix2 = std::string()) {
    if (!on_ready) return;
    int64_t lo = -1, hi = -1;
    for (const auto& s : m->slots) {
      const bool hit = s.key.compare(0, prefix.size(), prefix) == 0 || (!prefix2.empty() && s.key.compare(0, prefix2.size(), prefix2) == 0);
      if (!hit) continue;
      if (lo < 0) lo = s.offset;
      hi = s.offset + s.numel;
    }
    if (lo >= 0) on_ready(user, lo, hi - lo);
  };
  // ---- tail: y = out_proj(silu(P)), P = skip_proj(XS), XS = SK / sqrt(L) ----
  const float* dP = dy;
  if (m->has_out) {
    DMEL_TRY(launch_conv_wgrad(p.Q, dy, G("output_projection.conv.weight"), G("output_projection.conv.bias"), m->Cout, C, 1, 1, N, T, st));
    ConvRun r = run_1seg(dy, m->Cout, T, p.DQ, C, T, N);
    r.precision = prec;
    DMEL_TRY(launch_conv(m->out_dx, r, st));
    DMEL_TRY(launch_silu_bwd(p.DQ, p.P, p.DP, (int64_t)n, st));
    dP = p.DP;
  }
  DMEL_TRY(launch_conv_wgrad(p.XS, dP, G("skip_projection.conv.weight"), G("skip_projection.conv.bias"), C, C, 1, 1, N, T, st));
  {
    ConvRun r = run_1seg(dP, C, T, p.DZ, C, T, N);      // DZ as scratch: d XS
    r.precision = prec;
    DMEL_TRY(launch_conv(m->skip_dx, r, st));
    DMEL_TRY(launch_scale(p.DZ, p.GS, (float)(1.0 / std::sqrt((double)m->L)), (int64_t)n, st));   // d skip of every block
  }
  ready("skip_projection.", "output_projection.");
  // ---- blocks in reverse; gx = d loss / d x_{i+1}; x_L feeds nothing but the (discarded) last residual: gx starts at 0 ----
  float* gx = p.GXa;
  float* gx_prev = p.GXb;
  DMEL_HIP(hipMemsetAsync(gx, 0, n * sizeof(float), st));
  for (int i = m->L - 1; i >= 0; --i) {
    const std::string pk = "residual_layers." + std::to_string(i) + ".";
    const dmel_wavenet::TrainLayer& t = m->tl[i];
    const float* xi = p.X + (size_t)i * n;
    const float* pre = p.PRE + (size_t)i * 2 * n;
    const float* z = p.Z + (size_t)i * n;
    DMEL_TRY(launch_resskip_bwd(gx, p.GS, p.GO, p.GXS, N, C, T, st));
    DMEL_TRY(launch_conv_wgrad(z, p.GO, G(pk + "output_projection.conv.weight"), G(pk + "output_projection.conv.bias"), 2 * C, C, 1, 1, N,
                               T, st));
    {
      ConvRun r = run_1seg(p.GO, 2 * C, T, p.DZ, C, T, N);
      r.precision = prec;
      DMEL_TRY(launch_conv(t.out_dz, r, st));
    }
    DMEL_TRY(launch_gate_bwd(p.DZ, pre, p.DPRE, N, C, T, st));
    float* db = G(pk + "conv_layer.conv.bias");
    DMEL_TRY(launch_conv_wgrad(xi, p.DPRE, G(pk + "conv_layer.conv.weight"), db, 2 * C, C, 3, t.dil, N, T, st));
    if (Cc) {
      DMEL_TRY(launch_conv_wgrad(condition, p.DPRE, G(pk + "condition_projection.conv.weight"), nullptr, 2 * C, Cc, 1, 1, N, T, st));
      DMEL_HIP(hipMemcpyAsync(G(pk + "condition_projection.conv.bias"), db, (size_t)2 * C * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (dcondition) {
        ConvRun r = run_1seg(p.DPRE, 2 * C, T, dcondition, Cc, T, N);
        r.accumulate = (i != m->L - 1);
        r.precision = prec;
        DMEL_TRY(launch_conv(t.pre_dc, r, st));
      }
    }
    {
      ConvRun r = run_1seg(p.DPRE, 2 * C, T, gx_prev, C, T, N);     // d x_i = gx / sqrt2 + W^T d pre
      r.res = p.GXS; r.res_bs = (int64_t)C * T; r.res_cs = T;
      r.precision = prec;
      DMEL_TRY(launch_conv(t.pre_dx, r, st));
    }
    ready(pk);      // every gradient of block i is enqueued: its bucket can leave while blocks i-1 ... 0 still run
    std::swap(gx, gx_prev);
  }
  // ---- head: x_0 = silu(U), U = in_proj(x) ----
  if (m->has_in) {
    DMEL_TRY(launch_silu_bwd(gx, p.U, p.DP, (int64_t)n, st));
    DMEL_TRY(launch_conv_wgrad(x, p.DP, G("input_projection.conv.weight"), G("input_projection.conv.bias"), C, m->Cin, 1, 1, N, T, st));
    if (dx) {
      ConvRun r = run_1seg(p.DP, C, T, dx, m->Cin, T, N);
      r.precision = prec;
      DMEL_TRY(launch_conv(m->in_dx, r, st));
    }
  } else if (dx) {
    DMEL_HIP(hipMemcpyAsync(dx, gx, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  ready("input_projection.");
  return DMEL_OK;
}

// =====================================================================================================
// DownsampleFiniteScalarQuantize (is_dmel)          models/modules/dowmsample_fsq.py:124-147
// =====================================================================================================
namespace {
struct ConvNeXt {                // firefly.py:337-402
  std::string prefix;            // state-dict prefix of its nine tensors
  DevBuf dw_w, dw_b, ln_w, ln_b, gamma;
  WeightImage pw1, pw2;
  WeightImage pw1T, pw2T;        // training: transposed images, backward-data of the two Linear layers
};
int build_convnext(ConvNeXt& cx, const TensorStore& ts, const std::string& p, int C, bool train) {
  const HostTensor* dw = ts.need(p + "dwconv.weight", {C, 1, 7});
  const HostTensor* db = ts.need(p + "dwconv.bias", {C});
  const HostTensor* lw = ts.need(p + "norm.weight", {C});
  const HostTensor* lb = ts.need(p + "norm.bias", {C});
  const HostTensor* w1 = ts.need(p + "pwconv1.weight", {4 * C, C});
  const HostTensor* b1 = ts.need(p + "pwconv1.bias", {4 * C});
  const HostTensor* w2 = ts.need(p + "pwconv2.weight", {C, 4 * C});
  const HostTensor* b2 = ts.need(p + "pwconv2.bias", {C});
  const HostTensor* ga = ts.need(p + "gamma", {C});
  if (!dw || !db || !lw || !lb || !w1 || !b1 || !w2 || !b2 || !ga) return DMEL_EMISSING;
  cx.prefix = p;
  DMEL_TRY(upload_vec(cx.dw_w, dw->v)); DMEL_TRY(upload_vec(cx.dw_b, db->v));
  DMEL_TRY(upload_vec(cx.ln_w, lw->v)); DMEL_TRY(upload_vec(cx.ln_b, lb->v));
  DMEL_TRY(upload_vec(cx.gamma, ga->v));
  PackDesc d, e;
  d.mode = EPI_LINEAR; d.nseg = 1; d.C = 4 * C; d.seg[0].Cin = C;             // pwconv1, and W2^T: d v (C) -> d g (4C)
  e.mode = EPI_LINEAR; e.nseg = 1; e.C = C; e.seg[0].Cin = 4 * C;             // pwconv2, and W1^T: d u (4C) -> d h1 (C)
  ImageSrc s1, s2, s1T, s2T;
  s1.seg[0] = seg_rows(p + "pwconv1.weight", C); s1.b0 = p + "pwconv1.bias";
  s2.seg[0] = seg_rows(p + "pwconv2.weight", 4 * C); s2.b0 = p + "pwconv2.bias";
  DMEL_TRY(pack_image(cx.pw1, d, s1, ts));
  DMEL_TRY(pack_image(cx.pw2, e, s2, ts));
  if (!train) return DMEL_OK;
  s1T.seg[0] = seg_cols(p + "pwconv1.weight", C);
  s2T.seg[0] = seg_cols(p + "pwconv2.weight", 4 * C);
  DMEL_TRY(pack_image(cx.pw1T, e, s1T, ts));
  return pack_image(cx.pw2T, d, s2T, ts);
}
// the refresh of one block: five plain copies, two images (four when it trains)
int refresh_convnext(Refresh& r, ConvNeXt& cx, int C, bool train) {
  const std::string& p = cx.prefix;
  DMEL_TRY(r.add(cx.pw1)); DMEL_TRY(r.add(cx.pw2));
  DMEL_TRY(r.copy(cx.dw_w.as<float>(), p + "dwconv.weight", (size_t)C * 7)); DMEL_TRY(r.copy(cx.dw_b.as<float>(), p + "dwconv.bias", C));
  DMEL_TRY(r.copy(cx.ln_w.as<float>(), p + "norm.weight", C)); DMEL_TRY(r.copy(cx.ln_b.as<float>(), p + "norm.bias", C));
  DMEL_TRY(r.copy(cx.gamma.as<float>(), p + "gamma", C));
  if (train) { DMEL_TRY(r.add(cx.pw1T)); DMEL_TRY(r.add(cx.pw2T)); }
  return DMEL_OK;
}
// y = x + gamma * pwconv2(gelu(pwconv1(LN(dwconv(x)))))      x, y: (N, C, T); y may alias x; h1: (N,C,T), h2: (N,4C,T)
// len (nullable, N / len_div device int64): per-item form -- row n is an item of len[n / len_div] <= T columns.  The depthwise convolution
// pads each item with its own zeros, the pointwise convolutions are column-local, and h1, h2 and y come out zero behind the item; x is
// not read there by the depthwise taps or the staging (the residual load of a masked column is discarded, never stored).
// (tests/test_gpu_convnext_matrix.py mirrors the workspace order: h1 (N C T floats) at offset 0, h2 (4 N C T) directly behind it)
int run_convnext(const ConvNeXt& cx, const float* x, float* y, float* h1, float* h2, int N, int C, int64_t T, hipStream_t st,
                 const int64_t* len = nullptr, int len_div = 1) {
  DMEL_TRY(launch_dwconv_ln(x, h1, cx.dw_w.as<float>(), cx.dw_b.as<float>(), cx.ln_w.as<float>(), cx.ln_b.as<float>(), N, C, T, st, nullptr,
                            len, len_div));
  ConvRun a = run_1seg(h1, C, T, h2, 4 * C, T, N);
  a.act = ACT_GELU;
  a.seg[0].in_len = len; a.out_len = len; a.len_div = len_div;
  DMEL_TRY(launch_conv(cx.pw1, a, st));
  ConvRun b = run_1seg(h2, 4 * C, T, y, C, T, N);
  b.row_scale = cx.gamma.as<float>();
  b.res = x; b.res_bs = (int64_t)C * T; b.res_cs = T;
  b.seg[0].in_len = len; b.out_len = len; b.len_div = len_div;
  return launch_conv(cx.pw2, b, st);
}
}  // namespace

// ---- standalone ConvNeXtBlock handle (firefly.py:337-402), inference and training -----------------------------------
struct dmel_convnext : TrainHandle {
  int C = 0;
  ConvNeXt cx;
};

extern "C" int dmel_convnext_create(dmel_convnext** out, int dim) {
  DMEL_CHECK_ARG(out && dim > 0, "convnext_create: bad argument");
  auto* m = new dmel_convnext();
  m->C = dim;
  *out = m;
  return DMEL_OK;
}
extern "C" void dmel_convnext_destroy(dmel_convnext* m) { delete m; }
extern "C" int dmel_convnext_set_tensor(dmel_convnext* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  return train_set_tensor(m, key, data, shape, ndim);
}
extern "C" int dmel_convnext_set_train_precision(dmel_convnext* m, int precision) { return train_set_precision(m, "convnext", precision); }
extern "C" int dmel_convnext_enable_training(dmel_convnext* m, int on) { return train_enable(m, on); }
namespace {
// forward_train would run up to 494 channels and backward then fail in launch_ln_bwd with three gradients already written: a training
// handle is refused here, before any launch
int check_train_channels(const char* who, int C, bool train) {
  if (train && C > kLnBwdMaxC) {
    set_error("%s: a trainable ConvNeXt block has at most %d channels (the LayerNorm backward keeps two [C][33] fp32 tiles in the 64 KiB LDS), got %d",
              who, kLnBwdMaxC, C);
    return DMEL_EUNSUPPORTED;
  }
  return DMEL_OK;
}
// the nine gradient slots of a block, in the order of its state dict
void convnext_slots(TrainHandle& h, const std::string& p, int C) {
  h.add(p + "dwconv.weight", (int64_t)C * 7); h.add(p + "dwconv.bias", C); h.add(p + "norm.weight", C); h.add(p + "norm.bias", C);
  h.add(p + "pwconv1.weight", (int64_t)4 * C * C); h.add(p + "pwconv1.bias", 4 * C); h.add(p + "pwconv2.weight", (int64_t)4 * C * C);
  h.add(p + "pwconv2.bias", C); h.add(p + "gamma", C);
}
}  // namespace
extern "C" int dmel_convnext_finalize(dmel_convnext* m) {
  DMEL_CHECK_ARG(m, "NULL handle");
  m->ready = m->train_ready = false;      // until every image is packed: a finalize that fails leaves a handle that refuses to run
  DMEL_TRY(check_train_channels("convnext_finalize", m->C, m->train));
  DMEL_TRY(build_convnext(m->cx, m->ts, "", m->C, m->train));
  if (m->train) {
    m->clear_slots();
    convnext_slots(*m, "", m->C);
    m->train_ready = true;
  }
  m->ts.t.clear();
  m->ready = true;
  return DMEL_OK;
}
extern "C" size_t dmel_convnext_workspace_bytes(const dmel_convnext* m, int N, int64_t T) {
  if (!m || N <= 0 || T <= 0) return 0;
  return align_up((size_t)5 * N * m->C * T * sizeof(float), 256);
}
extern "C" int dmel_convnext_forward(const dmel_convnext* m, const float* x, float* y, int N, int64_t T, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(m && x && y && workspace, "convnext_forward: NULL argument");
  if (!m->ready) { set_error("convnext_forward: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(N > 0 && T > 0 && workspace_bytes >= dmel_convnext_workspace_bytes(m, N, T), "convnext_forward: bad shape or workspace");
  float* h1 = reinterpret_cast<float*>(workspace);
  return run_convnext(m->cx, x, y, h1, h1 + (size_t)N * m->C * T, N, m->C, T, (hipStream_t)stream);
}
extern "C" int dmel_convnext_forward_items(const dmel_convnext* m, const float* x, const int64_t* lengths_dev, float* y, int N, int64_t T,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(m && x && lengths_dev && y && workspace, "convnext_forward_items: NULL argument");
  if (!m->ready) { set_error("convnext_forward_items: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(N > 0 && T > 0 && workspace_bytes >= dmel_convnext_workspace_bytes(m, N, T), "convnext_forward_items: bad shape or workspace");
  float* h1 = reinterpret_cast<float*>(workspace);
  return run_convnext(m->cx, x, y, h1, h1 + (size_t)N * m->C * T, N, m->C, T, (hipStream_t)stream, lengths_dev, 1);
}

namespace {
struct CxPlan { float *H0, *H1, *U, *G, *V, *DV, *DG, *DH1, *DH0; size_t n, bytes; };
// (tests/test_gpu_convnext_matrix.py mirrors this order and the 256-byte alignment of every take)
CxPlan cx_plan_at(Arena& a, size_t n) {
  CxPlan p{};
  p.n = n;
  p.H0 = a.take<float>(n); p.H1 = a.take<float>(n); p.U = a.take<float>(4 * n); p.G = a.take<float>(4 * n); p.V = a.take<float>(n);
  p.DV = a.take<float>(n); p.DG = a.take<float>(4 * n); p.DH1 = a.take<float>(n); p.DH0 = a.take<float>(n);
  return p;
}
CxPlan cx_plan(const dmel_convnext* m, int N, int64_t T, void* ws) {
  Arena a(ws, (size_t)-1);
  CxPlan p = cx_plan_at(a, (size_t)N * m->C * T);
  p.bytes = align_up(a.off, 256);
  return p;
}
struct CxGrads { float *dw_w, *dw_b, *ln_w, *ln_b, *w1, *b1, *w2, *b2, *gamma; };
CxGrads cx_grads(const TrainHandle& h, float* grads, const std::string& p) {
  auto G = [&](const char* k) { return grads + h.offset_of(p + k); };
  return CxGrads{G("dwconv.weight"), G("dwconv.bias"), G("norm.weight"), G("norm.bias"), G("pwconv1.weight"), G("pwconv1.bias"),
                 G("pwconv2.weight"), G("pwconv2.bias"), G("gamma")};
}

// firefly.py:383-402 unfused, keeping the pre-norm, normed, pre-GELU, post-GELU and pre-scale tensors for backward
int convnext_train_fwd(const ConvNeXt& cx, const CxPlan& p, const float* x, float* y, int N, int C, int64_t T, hipStream_t st) {
  DMEL_TRY(launch_dwconv_ln(x, p.H1, cx.dw_w.as<float>(), cx.dw_b.as<float>(), cx.ln_w.as<float>(), cx.ln_b.as<float>(), N, C, T, st, p.H0));
  ConvRun a = run_1seg(p.H1, C, T, p.U, 4 * C, T, N);
  DMEL_TRY(launch_conv(cx.pw1, a, st));
  DMEL_TRY(launch_gelu_fwd(p.U, p.G, (int64_t)(4 * p.n), st));
  ConvRun b = run_1seg(p.G, 4 * C, T, p.V, C, T, N);
  DMEL_TRY(launch_conv(cx.pw2, b, st));
  return launch_layerscale_res_fwd(x, p.V, cx.gamma.as<float>(), y, N, C, T, st);
}
int convnext_bwd(const ConvNeXt& cx, const CxPlan& p, const CxGrads& g, const float* x, const float* dy, float* dx, int N, int C, int64_t T,
                 hipStream_t st) {
  DMEL_TRY(launch_layerscale_bwd(dy, p.V, cx.gamma.as<float>(), p.DV, g.gamma, N, C, T, st));          // y = x + gamma * V
  DMEL_TRY(launch_conv_wgrad(p.G, p.DV, g.w2, g.b2, C, 4 * C, 1, 1, N, T, st));                         // V = pwconv2(G)
  {
    ConvRun r = run_1seg(p.DV, C, T, p.DG, 4 * C, T, N);
    DMEL_TRY(launch_conv(cx.pw2T, r, st));
  }
  DMEL_TRY(launch_gelu_bwd(p.DG, p.U, p.DG, (int64_t)(4 * p.n), st));                                   // G = gelu(U); d U overwrites d G
  DMEL_TRY(launch_conv_wgrad(p.H1, p.DG, g.w1, g.b1, 4 * C, C, 1, 1, N, T, st));                        // U = pwconv1(H1)
  {
    ConvRun r = run_1seg(p.DG, 4 * C, T, p.DH1, C, T, N);
    DMEL_TRY(launch_conv(cx.pw1T, r, st));
  }
  // H1 = LayerNorm(H0), H0 = dwconv(x); dx = dy (identity path) + dwconv^T(d H0)
  DMEL_TRY(launch_ln_bwd(p.DH1, p.H0, cx.ln_w.as<float>(), p.DH0, g.ln_w, g.ln_b, N, C, T, st));
  return launch_dwconv_bwd(p.DH0, x, cx.dw_w.as<float>(), dy, dx, g.dw_w, g.dw_b, N, C, T, st);
}
}  // namespace

extern "C" size_t dmel_convnext_train_workspace_bytes(const dmel_convnext* m, int N, int64_t T) {
  if (!m || N <= 0 || T <= 0) return 0;
  return cx_plan(m, N, T, nullptr).bytes;
}
extern "C" int64_t dmel_convnext_grad_floats(const dmel_convnext* m) { return train_grad_floats(m); }
extern "C" int dmel_convnext_grad_slot(const dmel_convnext* m, const char* key, int64_t* offset, int64_t* numel) {
  return train_grad_slot(m, "convnext", "a parameter of ConvNeXtBlock", key, offset, numel);
}

extern "C" int dmel_convnext_forward_train(const dmel_convnext* m, const float* x, float* y, int N, int64_t T, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(m ? m->train_precision : 0);
  DMEL_CHECK_ARG(m && x && y && workspace, "convnext_forward_train: NULL argument");
  if (!m->ready || !m->train_ready) { set_error("convnext_forward_train: enable_training + finalize first"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(N > 0 && T > 0, "convnext_forward_train: bad shape");
  const CxPlan p = cx_plan(m, N, T, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "convnext_forward_train: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  return convnext_train_fwd(m->cx, p, x, y, N, m->C, T, (hipStream_t)stream);
}

extern "C" int dmel_convnext_backward(const dmel_convnext* m, const float* x, const float* dy, float* dx, float* grads, int N, int64_t T,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(m ? m->train_precision : 0);
  DMEL_CHECK_ARG(m && x && dy && dx && grads && workspace, "convnext_backward: NULL argument");
  if (!m->ready || !m->train_ready) { set_error("convnext_backward: enable_training + finalize first"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(N > 0 && T > 0, "convnext_backward: bad shape");
  const CxPlan p = cx_plan(m, N, T, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "convnext_backward: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  return convnext_bwd(m->cx, p, cx_grads(*m, grads, ""), x, dy, dx, N, m->C, T, (hipStream_t)stream);
}

struct dmel_quantizer : TrainHandle {
  int dim, G, Cg, D, nf;
  int factors[4];
  int levels[4];
  FsqConst fk;
  // per stage: the k2s2 conv / transposed conv with its ConvNeXt block, and (training) their backward-data images
  struct Stage { WeightImage down, up, down_dx, up_dx; ConvNeXt down_cx, up_cx; };
  std::vector<Stage> stage;
  DevBuf w_in, b_in, w_out, b_out;
};

extern "C" int dmel_quantizer_create(dmel_quantizer** out, int input_dim, int n_groups, const int* levels, int n_levels,
                                     const int* downsample_factor, int n_factors, int fsq_prebound) {
  DMEL_CHECK_ARG(out && levels && downsample_factor, "NULL argument");
  DMEL_CHECK_ARG(n_groups > 0 && input_dim > 0 && input_dim % n_groups == 0, "quantizer: input_dim %d not divisible by groups %d",
                 input_dim, n_groups);
  DMEL_CHECK_ARG(n_factors >= 1 && n_factors <= 4, "quantizer: 1..4 downsample stages supported");
  for (int i = 0; i < n_factors; ++i)
    if (downsample_factor[i] != 2) {
      set_error("quantizer: downsample factor %d unsupported (only 2)", downsample_factor[i]);
      return DMEL_EUNSUPPORTED;
    }
  auto* q = new dmel_quantizer();
  q->dim = input_dim; q->G = n_groups; q->Cg = input_dim / n_groups; q->D = n_levels; q->nf = n_factors;
  for (int i = 0; i < n_factors; ++i) q->factors[i] = downsample_factor[i];
  int rc = make_fsq_const(q->fk, levels, n_levels, fsq_prebound);
  if (rc != DMEL_OK) { delete q; return rc; }
  for (int i = 0; i < n_levels; ++i) q->levels[i] = levels[i];
  *out = q;
  return DMEL_OK;
}
extern "C" int dmel_quantizer_set_strict(dmel_quantizer* q, int on) {
  DMEL_CHECK_ARG(q, "NULL handle");
  q->fk.strict = on != 0;
  return DMEL_OK;
}
extern "C" void dmel_quantizer_destroy(dmel_quantizer* q) { delete q; }
extern "C" int dmel_quantizer_set_tensor(dmel_quantizer* q, const char* key, const float* data, const int64_t* shape, int ndim) {
  return train_set_tensor(q, key, data, shape, ndim);
}

extern "C" int dmel_quantizer_finalize(dmel_quantizer* q) {
  DMEL_CHECK_ARG(q, "NULL handle");
  q->ready = q->train_ready = false;      // until every image is packed: a finalize that fails leaves a handle that refuses to run
  const int C = q->Cg, G = q->G, D = q->D;
  DMEL_TRY(check_train_channels("quantizer_finalize", C, q->train));
  q->stage.clear();
  q->stage.resize(q->nf);
  q->clear_slots();
  PackDesc k2s2, k2s2T;
  k2s2.mode = EPI_LINEAR; k2s2.nseg = 2; k2s2.C = C;                   // Conv1d(k=2, stride=2): two 1-tap segments reading x[2s] and x[2s+1]
  for (int s = 0; s < 2; ++s) { k2s2.seg[s].Cin = C; k2s2.seg[s].tstride = 2; k2s2.seg[s].toff = s; }
  k2s2T.mode = EPI_LINEAR; k2s2T.nseg = 1; k2s2T.C = C; k2s2T.phases = 2; k2s2T.seg[0].Cin = C;      // its transpose: phase-major rows
  // the two views of a (C, C, 2) weight: rows as they lie with tap sg of segment sg, value(sg, row, ci) = w[(row*C + ci)*2 + sg];
  // and phase-major rows over the transpose, value(row = (ph, co), ci) = w[(ci*C + co)*2 + ph]
  auto strided = [&](const std::string& key) {
    ImageSrc v;
    for (int sg = 0; sg < 2; ++sg) { v.seg[sg].key = key; v.seg[sg].off = sg; v.seg[sg].rs = 2 * C; v.seg[sg].cs = 2; }
    return v;
  };
  auto phased = [&](const std::string& key) {
    ImageSrc v;
    v.seg[0].key = key; v.seg[0].rs = 2; v.seg[0].cs = 2 * C; v.seg[0].ps = 1; v.seg[0].pC = C;
    return v;
  };
  for (int i = 0; i < q->nf; ++i) {
    dmel_quantizer::Stage& sg = q->stage[i];
    const std::string pd = "downsample." + std::to_string(i) + ".", pu = "upsample." + std::to_string(i) + ".";
    for (int up = 0; up < 2; ++up) {
      const std::string& p = up ? pu : pd;
      const HostTensor* w = q->ts.need(p + "0.weight", {C, C, 2});
      const HostTensor* b = q->ts.need(p + "0.bias", {C});
      if (!w || !b) return DMEL_EMISSING;
      // upsample.{i}.0 = ConvTranspose1d, weight (Cin, Cout, 2): out[2q+ph] = W[:, :, ph]^T x[q], one bias per output channel for both phases
      ImageSrc src = up ? phased(p + "0.weight") : strided(p + "0.weight");
      src.b0 = p + "0.bias";
      src.bias_mod = up ? C : 0;
      DMEL_TRY(pack_image(up ? sg.up : sg.down, up ? k2s2T : k2s2, src, q->ts));
      DMEL_TRY(build_convnext(up ? sg.up_cx : sg.down_cx, q->ts, p + "1.", C, q->train));
    }
    if (!q->train) continue;
    // d x[ci, 2q + k] = sum_co W[co, ci, k] d y[co, q]: a k2s2 transposed conv;  d x[ci, q] = sum_{co, k} W[ci, co, k] d y[co, 2q + k]: a k2s2 conv
    DMEL_TRY(pack_image(sg.down_dx, k2s2T, phased(pd + "0.weight"), q->ts));
    DMEL_TRY(pack_image(sg.up_dx, k2s2, strided(pu + "0.weight"), q->ts));
    for (const std::string* p : {&pd, &pu}) {
      q->add(*p + "0.weight", (int64_t)C * C * 2); q->add(*p + "0.bias", C);
      convnext_slots(*q, *p + "1.", C);
    }
  }
  std::vector<float> wi((size_t)G * D * C), bi((size_t)G * D), wo((size_t)G * C * D), bo((size_t)G * C);
  for (int g = 0; g < G; ++g) {
    const std::string p = "residual_fsq.rvqs." + std::to_string(g) + ".";
    const HostTensor* a = q->ts.need(p + "project_in.weight", {D, C});
    const HostTensor* ab = q->ts.need(p + "project_in.bias", {D});
    const HostTensor* o = q->ts.need(p + "project_out.weight", {C, D});
    const HostTensor* ob = q->ts.need(p + "project_out.bias", {C});
    if (!a || !ab || !o || !ob) return DMEL_EMISSING;
    std::copy(a->v.begin(), a->v.end(), wi.begin() + (size_t)g * D * C);
    std::copy(ab->v.begin(), ab->v.end(), bi.begin() + (size_t)g * D);
    std::copy(o->v.begin(), o->v.end(), wo.begin() + (size_t)g * C * D);
    std::copy(ob->v.begin(), ob->v.end(), bo.begin() + (size_t)g * C);
  }
  DMEL_TRY(upload_vec(q->w_in, wi)); DMEL_TRY(upload_vec(q->b_in, bi));
  DMEL_TRY(upload_vec(q->w_out, wo)); DMEL_TRY(upload_vec(q->b_out, bo));
  if (q->train) {
    // FSQ parameter gradients come out in the packed (G, ...) layouts: group g's tensor is the g-th block of each region
    const int64_t o_wi = q->grad_floats, o_bi = o_wi + (int64_t)G * D * C, o_wo = o_bi + (int64_t)G * D, o_bo = o_wo + (int64_t)G * C * D;
    for (int g = 0; g < G; ++g) {
      const std::string p = "residual_fsq.rvqs." + std::to_string(g) + ".";
      q->slots.push_back({p + "project_in.weight", o_wi + (int64_t)g * D * C, (int64_t)D * C});
      q->slots.push_back({p + "project_in.bias", o_bi + (int64_t)g * D, D});
      q->slots.push_back({p + "project_out.weight", o_wo + (int64_t)g * C * D, (int64_t)C * D});
      q->slots.push_back({p + "project_out.bias", o_bo + (int64_t)g * C, C});
    }
    q->add("#fsq.w_in", (int64_t)G * D * C);
    q->add("#fsq.b_in", (int64_t)G * D);
    q->add("#fsq.w_out", (int64_t)G * C * D);
    q->add("#fsq.b_out", (int64_t)G * C);
    q->train_ready = true;
  }
  q->ts.t.clear();
  q->ready = true;
  return DMEL_OK;
}

extern "C" int dmel_quantizer_set_train_precision(dmel_quantizer* q, int precision) { return train_set_precision(q, "quantizer", precision); }
extern "C" int dmel_quantizer_enable_training(dmel_quantizer* q, int on) { return train_enable(q, on); }

static size_t quantizer_plan(const dmel_quantizer* q, int B, int64_t Tmax, void* ws, float** a, float** b, float** h1, float** h2) {
  Arena ar(ws, (size_t)-1);
  const size_t n = (size_t)B * q->G * q->Cg * Tmax;
  float* pa = ar.take<float>(n);
  float* pb = ar.take<float>(n);
  float* p1 = ar.take<float>(n);
  float* p2 = ar.take<float>(4 * n);
  if (a) { *a = pa; *b = pb; *h1 = p1; *h2 = p2; }
  return align_up(ar.off, 256);
}

extern "C" size_t dmel_quantizer_workspace_bytes(const dmel_quantizer* q, int B, int64_t T) {
  if (!q || B <= 0 || T <= 0) return 0;
  return quantizer_plan(q, B, T, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int dmel_quantizer_encode(const dmel_quantizer* q, const float* z, int32_t* ids, float* prequant, int B, int64_t T,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return dmel_quantizer_encode_ex(q, z, ids, prequant, nullptr, B, T, workspace, workspace_bytes, stream);
}

// Per-item form of both directions (lengths != nullptr): one launch expands the lengths into a table of nf + 1 stages at the end of the
// workspace, and every layer sees each item's own end from the row of its stage -- the k2s2 convolutions and the pointwise ones through
// SegRun::in_len / ConvRun::out_len (columns behind an item staged as zeros, results behind it stored as zeros), the depthwise k = 7
// convolution and FSQ through their item forms.  Every buffer is therefore zero behind each item after every launch, nothing behind an
// item's length in the caller's tensor is read, and the columns in front of it go through the same arithmetic, in the same order, as a
// call on the item alone.
static size_t quantizer_items_plan(const dmel_quantizer* q, int B, int64_t Tmax, void* ws, float** a, float** b, float** h1, float** h2,
                                   int64_t** tab) {
  const size_t off = quantizer_plan(q, B, Tmax, ws, a, b, h1, h2);
  if (tab) *tab = reinterpret_cast<int64_t*>(static_cast<char*>(ws) + off);
  return off + align_up((size_t)(q->nf + 1) * B * sizeof(int64_t), 256);
}

extern "C" size_t dmel_quantizer_items_workspace_bytes(const dmel_quantizer* q, int B, int64_t T) {
  if (!q || B <= 0 || T <= 0) return 0;
  return quantizer_items_plan(q, B, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

static int quantizer_encode_run(const dmel_quantizer* q, const float* z, const int64_t* lengths, int32_t* ids, float* prequant,
                                float* latents, int B, int64_t T, void* workspace, size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(q && z && ids && workspace, "quantizer_encode: NULL argument");
  if (!q->ready) { set_error("quantizer_encode: handle not finalized"); return DMEL_EMISSING; }
  int64_t Tq = T;
  for (int i = 0; i < q->nf; ++i) Tq /= 2;
  DMEL_CHECK_ARG(B > 0 && Tq > 0, "quantizer_encode: sequence too short for the downsampling (T=%lld)", (long long)T);
  float *pa, *pb, *h1, *h2;
  int64_t* tab = nullptr;
  const size_t need = lengths ? quantizer_items_plan(q, B, T, workspace, &pa, &pb, &h1, &h2, &tab)
                              : quantizer_plan(q, B, T, workspace, &pa, &pb, &h1, &h2);
  DMEL_CHECK_ARG(workspace_bytes >= need, "quantizer_encode: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int N = B * q->G, C = q->Cg;
  if (lengths) DMEL_TRY(launch_stage_lengths(lengths, tab, B, T, q->nf + 1, /*down=*/1, st));      // len, len / 2, len / 4
  auto len_at = [&](int stage) -> const int64_t* { return lengths ? tab + (size_t)stage * B : nullptr; };
  const float* cur = z;
  int64_t Tc = T;
  float* bufs[2] = {pa, pb};
  for (int i = 0; i < q->nf; ++i) {  // dowmsample_fsq.py:49-62
    const int64_t Tn = Tc / 2;
    float* o = bufs[i & 1];
    ConvRun r;
    for (int s = 0; s < 2; ++s) {
      r.seg[s].x = cur; r.seg[s].bstride = (int64_t)C * Tc; r.seg[s].cstride = Tc; r.seg[s].Tin = Tc;
      r.seg[s].in_len = len_at(i);
    }
    r.B = N; r.Tcols = Tn; r.y = o; r.y_bs = (int64_t)C * Tn; r.y_cs = Tn; r.Tout = Tn;
    r.out_len = len_at(i + 1); r.len_div = lengths ? q->G : 1;
    DMEL_TRY(launch_conv(q->stage[i].down, r, st));
    DMEL_TRY(run_convnext(q->stage[i].down_cx, o, o, h1, h2, N, C, Tn, st, len_at(i + 1), lengths ? q->G : 1));
    cur = o;
    Tc = Tn;
  }
  if (latents) DMEL_HIP(hipMemcpyAsync(latents, cur, (size_t)N * C * Tc * sizeof(float), hipMemcpyDeviceToDevice, st));
  // "(b g) f t -> b (g f) t" is a view; FSQ per group (dowmsample_fsq.py:127-132)
  return launch_fsq_encode(cur, q->w_in.as<float>(), q->b_in.as<float>(), ids, prequant, q->fk, B, q->G, C, Tc, st, len_at(q->nf));
}

extern "C" int dmel_quantizer_encode_ex(const dmel_quantizer* q, const float* z, int32_t* ids, float* prequant, float* latents, int B,
                                        int64_t T, void* workspace, size_t workspace_bytes, void* stream) {
  return quantizer_encode_run(q, z, nullptr, ids, prequant, latents, B, T, workspace, workspace_bytes, stream);
}

extern "C" int dmel_quantizer_encode_items(const dmel_quantizer* q, const float* z, const int64_t* lengths_dev, int32_t* ids, int B,
                                           int64_t T, void* workspace, size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(lengths_dev, "quantizer_encode_items: NULL lengths");
  return quantizer_encode_run(q, z, lengths_dev, ids, nullptr, nullptr, B, T, workspace, workspace_bytes, stream);
}

static int quantizer_decode_run(const dmel_quantizer* q, const int32_t* ids, const int64_t* lengths, float* zout, int B, int64_t T4,
                                void* workspace, size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(q && ids && zout && workspace, "quantizer_decode: NULL argument");
  if (!q->ready) { set_error("quantizer_decode: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(B > 0 && T4 > 0, "quantizer_decode: bad shape");
  int64_t Tfull = T4;
  for (int i = 0; i < q->nf; ++i) Tfull *= 2;
  float *pa, *pb, *h1, *h2;
  int64_t* tab = nullptr;
  const size_t need = lengths ? quantizer_items_plan(q, B, Tfull, workspace, &pa, &pb, &h1, &h2, &tab)
                              : quantizer_plan(q, B, Tfull, workspace, &pa, &pb, &h1, &h2);
  DMEL_CHECK_ARG(workspace_bytes >= need, "quantizer_decode: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int N = B * q->G, C = q->Cg;
  if (lengths) DMEL_TRY(launch_stage_lengths(lengths, tab, B, T4, q->nf + 1, /*down=*/0, st));      // len, 2 len, 4 len
  auto len_at = [&](int stage) -> const int64_t* { return lengths ? tab + (size_t)stage * B : nullptr; };
  DMEL_TRY(launch_fsq_decode(ids, q->w_out.as<float>(), q->b_out.as<float>(), pa, q->fk, B, q->G, C, T4, st, len_at(0)));
  const float* cur = pa;
  int64_t Tc = T4;
  float* bufs[2] = {pb, pa};
  for (int j = 0; j < q->nf; ++j) {  // dowmsample_fsq.py:64-77 (upsample.{j}: reversed factor order, all factors are 2)
    const int64_t Tn = Tc * 2;
    float* o = (j == q->nf - 1) ? zout : bufs[j & 1];
    ConvRun r = run_1seg(cur, C, Tc, o, C, Tn, N);
    r.Tcols = Tc; r.out_tstride = 2; r.Tout = Tn;
    r.seg[0].in_len = len_at(j); r.out_len = len_at(j + 1); r.len_div = lengths ? q->G : 1;      // out_len counts OUTPUT columns (conv_dev.h)
    DMEL_TRY(launch_conv(q->stage[j].up, r, st));
    DMEL_TRY(run_convnext(q->stage[j].up_cx, o, o, h1, h2, N, C, Tn, st, len_at(j + 1), lengths ? q->G : 1));
    cur = o;
    Tc = Tn;
  }
  return DMEL_OK;
}

extern "C" int dmel_quantizer_decode(const dmel_quantizer* q, const int32_t* ids, float* zout, int B, int64_t T4, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return quantizer_decode_run(q, ids, nullptr, zout, B, T4, workspace, workspace_bytes, stream);
}

extern "C" int dmel_quantizer_decode_items(const dmel_quantizer* q, const int32_t* ids, const int64_t* lengths_dev, float* zout, int B,
                                           int64_t T4, void* workspace, size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(lengths_dev, "quantizer_decode_items: NULL lengths");
  return quantizer_decode_run(q, ids, lengths_dev, zout, B, T4, workspace, workspace_bytes, stream);
}

// Re-pack every weight image and parameter buffer of a finalized quantiser from device tensors (after an optimiser step).
extern "C" int dmel_quantizer_refresh(dmel_quantizer* q, int n, const char* const* keys, const float* const* device_tensors, void* stream) {
  DMEL_CHECK_ARG(q && keys && device_tensors && n > 0, "quantizer_refresh: bad argument");
  if (!q->ready) { set_error("quantizer_refresh: handle not finalized"); return DMEL_EMISSING; }
  Refresh r("quantizer_refresh", stream);
  DMEL_TRY(r.open(n, keys, device_tensors));
  const int C = q->Cg, D = q->D;
  for (auto& sg : q->stage) {
    DMEL_TRY(r.add(sg.down)); DMEL_TRY(refresh_convnext(r, sg.down_cx, C, q->train_ready));
    DMEL_TRY(r.add(sg.up)); DMEL_TRY(refresh_convnext(r, sg.up_cx, C, q->train_ready));
    if (q->train_ready) { DMEL_TRY(r.add(sg.down_dx)); DMEL_TRY(r.add(sg.up_dx)); }
  }
  for (int g = 0; g < q->G; ++g) {
    const std::string p = "residual_fsq.rvqs." + std::to_string(g) + ".";
    DMEL_TRY(r.copy(q->w_in.as<float>() + (size_t)g * D * C, p + "project_in.weight", (size_t)D * C));
    DMEL_TRY(r.copy(q->b_in.as<float>() + (size_t)g * D, p + "project_in.bias", D));
    DMEL_TRY(r.copy(q->w_out.as<float>() + (size_t)g * C * D, p + "project_out.weight", (size_t)C * D));
    DMEL_TRY(r.copy(q->b_out.as<float>() + (size_t)g * C, p + "project_out.bias", C));
  }
  return r.run();
}

// ---- quantiser training path: DownsampleFiniteScalarQuantize.forward (dowmsample_fsq.py:86-122) and its backward ----------
namespace {
struct QStage { float* in; float* conv; CxPlan cx; int64_t Tin, Tout; };      // input of the (transposed) conv, its output = ConvNeXt input
struct QPlan {
  QStage down[4], up[4];
  float *lat, *fsq_out, *ga, *gb, *scratch;
  int32_t* ids;
  int64_t T4;
  size_t bytes;
};
QPlan q_plan(const dmel_quantizer* q, int B, int64_t T, void* ws) {
  QPlan p{};
  Arena a(ws, (size_t)-1);
  const size_t NC = (size_t)B * q->G * q->Cg;
  int64_t Tc = T;
  for (int i = 0; i < q->nf; ++i) {
    const int64_t Tn = Tc / 2;
    p.down[i].Tin = Tc; p.down[i].Tout = Tn;
    p.down[i].in = i == 0 ? nullptr : a.take<float>(NC * Tc);     // stage 0 reads the caller's z
    p.down[i].conv = a.take<float>(NC * Tn);
    p.down[i].cx = cx_plan_at(a, NC * Tn);
    Tc = Tn;
  }
  p.T4 = Tc;
  p.lat = a.take<float>(NC * Tc);
  p.ids = a.take<int32_t>((size_t)B * q->G * Tc);
  p.fsq_out = a.take<float>(NC * Tc);
  p.scratch = a.take<float>((size_t)2 * B * q->G * Tc * q->D);
  for (int j = 0; j < q->nf; ++j) {
    const int64_t Tn = Tc * 2;
    p.up[j].Tin = Tc; p.up[j].Tout = Tn;
    p.up[j].in = j == 0 ? p.fsq_out : a.take<float>(NC * Tc);
    p.up[j].conv = a.take<float>(NC * Tn);
    p.up[j].cx = cx_plan_at(a, NC * Tn);
    Tc = Tn;
  }
  p.ga = a.take<float>(NC * T);
  p.gb = a.take<float>(NC * T);
  p.bytes = align_up(a.off, 256);
  return p;
}
}  // namespace

extern "C" size_t dmel_quantizer_train_workspace_bytes(const dmel_quantizer* q, int B, int64_t T) {
  if (!q || B <= 0 || T <= 0) return 0;
  return q_plan(q, B, T, nullptr).bytes;
}
extern "C" int64_t dmel_quantizer_grad_floats(const dmel_quantizer* q) { return train_grad_floats(q); }
extern "C" int dmel_quantizer_grad_slot(const dmel_quantizer* q, const char* key, int64_t* offset, int64_t* numel) {
  return train_grad_slot(q, "quantizer", "a trained parameter of this quantiser", key, offset, numel);
}

// z (B*G, Cg, T) -> zq (B*G, Cg, T) [= (B, G*Cg, T)], ids (B, G, T4), latents (B*G, Cg, T4); zq is zero-padded from 2^nf * T4 to T
// (left = diff / 2) exactly as dowmsample_fsq.py:113-120.
extern "C" int dmel_quantizer_forward_train(const dmel_quantizer* q, const float* z, float* zq, int32_t* ids, float* latents, int B,
                                            int64_t T, void* workspace, size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(q ? q->train_precision : 0);
  DMEL_CHECK_ARG(q && z && zq && workspace, "quantizer_forward_train: NULL argument");
  if (!q->ready || !q->train_ready) { set_error("quantizer_forward_train: enable_training + finalize first"); return DMEL_EMISSING; }
  const QPlan p = q_plan(q, B, T, workspace);
  DMEL_CHECK_ARG(B > 0 && p.T4 > 0, "quantizer_forward_train: sequence too short for the downsampling (T=%lld)", (long long)T);
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "quantizer_forward_train: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int N = B * q->G, C = q->Cg;
  const size_t NC = (size_t)N * C;
  const float* cur = z;
  for (int i = 0; i < q->nf; ++i) {
    const QStage& sgq = p.down[i];
    ConvRun r;
    for (int s = 0; s < 2; ++s) { r.seg[s].x = cur; r.seg[s].bstride = (int64_t)C * sgq.Tin; r.seg[s].cstride = sgq.Tin; r.seg[s].Tin = sgq.Tin; }
    r.B = N; r.Tcols = sgq.Tout; r.y = sgq.conv; r.y_bs = (int64_t)C * sgq.Tout; r.y_cs = sgq.Tout; r.Tout = sgq.Tout;
    DMEL_TRY(launch_conv(q->stage[i].down, r, st));
    float* o = (i == q->nf - 1) ? p.lat : p.down[i + 1].in;
    DMEL_TRY(convnext_train_fwd(q->stage[i].down_cx, sgq.cx, sgq.conv, o, N, C, sgq.Tout, st));
    cur = o;
  }
  DMEL_TRY(launch_fsq_encode(p.lat, q->w_in.as<float>(), q->b_in.as<float>(), p.ids, nullptr, q->fk, B, q->G, C, p.T4, st));
  DMEL_TRY(launch_fsq_decode(p.ids, q->w_out.as<float>(), q->b_out.as<float>(), p.fsq_out, q->fk, B, q->G, C, p.T4, st));
  if (ids) DMEL_HIP(hipMemcpyAsync(ids, p.ids, (size_t)B * q->G * p.T4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (latents) DMEL_HIP(hipMemcpyAsync(latents, p.lat, NC * p.T4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  cur = p.fsq_out;
  for (int j = 0; j < q->nf; ++j) {
    const QStage& sgq = p.up[j];
    ConvRun r = run_1seg(cur, C, sgq.Tin, sgq.conv, C, sgq.Tout, N);
    r.Tcols = sgq.Tin; r.out_tstride = 2; r.Tout = sgq.Tout;
    DMEL_TRY(launch_conv(q->stage[j].up, r, st));
    float* o = (j == q->nf - 1) ? p.ga : p.up[j + 1].in;
    DMEL_TRY(convnext_train_fwd(q->stage[j].up_cx, sgq.cx, sgq.conv, o, N, C, sgq.Tout, st));
    cur = o;
  }
  const int64_t Tfull = p.up[q->nf - 1].Tout, diff = T - Tfull, left = diff / 2;
  if (diff == 0) {
    DMEL_HIP(hipMemcpyAsync(zq, p.ga, NC * T * sizeof(float), hipMemcpyDeviceToDevice, st));
  } else {
    DMEL_HIP(hipMemsetAsync(zq, 0, NC * T * sizeof(float), st));
    DMEL_HIP(hipMemcpy2DAsync(zq + left, (size_t)T * sizeof(float), p.ga, (size_t)Tfull * sizeof(float), (size_t)Tfull * sizeof(float), NC,
                              hipMemcpyDeviceToDevice, st));
  }
  return DMEL_OK;
}

extern "C" int dmel_quantizer_backward(const dmel_quantizer* q, const float* z, const float* dzq, float* dz, float* grads, int B, int64_t T,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(q ? q->train_precision : 0);
  DMEL_CHECK_ARG(q && z && dzq && dz && grads && workspace, "quantizer_backward: NULL argument");
  if (!q->ready || !q->train_ready) { set_error("quantizer_backward: enable_training + finalize first"); return DMEL_EMISSING; }
  const QPlan p = q_plan(q, B, T, workspace);
  DMEL_CHECK_ARG(B > 0 && p.T4 > 0 && workspace_bytes >= p.bytes, "quantizer_backward: bad shape or workspace");
  hipStream_t st = (hipStream_t)stream;
  const int N = B * q->G, C = q->Cg;
  const size_t NC = (size_t)N * C;
  ClearedRange cleared(grads, (size_t)q->grad_floats * sizeof(float), st);
  DMEL_TRY(cleared.error());
  const int64_t Tfull = p.up[q->nf - 1].Tout, diff = T - Tfull, left = diff / 2;
  // un-pad: gradient of the cropped region only
  float* g = p.gb;
  if (diff == 0) {
    DMEL_HIP(hipMemcpyAsync(g, dzq, NC * T * sizeof(float), hipMemcpyDeviceToDevice, st));
  } else {
    DMEL_HIP(hipMemcpy2DAsync(g, (size_t)Tfull * sizeof(float), dzq + left, (size_t)T * sizeof(float), (size_t)Tfull * sizeof(float), NC,
                              hipMemcpyDeviceToDevice, st));
  }
  float* other = p.ga;
  for (int j = q->nf - 1; j >= 0; --j) {      // upsample.{j}: ConvTranspose1d(k2, s2) -> ConvNeXtBlock
    const QStage& sgq = p.up[j];
    const std::string pu = "upsample." + std::to_string(j) + ".";
    DMEL_TRY(convnext_bwd(q->stage[j].up_cx, sgq.cx, cx_grads(*q, grads, pu + "1."), sgq.conv, g, other, N, C,
                          sgq.Tout, st));
    std::swap(g, other);                       // g = d (transposed conv output), length Tout
    float* dw = grads + q->offset_of(pu + "0.weight");
    DMEL_TRY(zero_unless_cleared(dw, (size_t)C * C * 2 * sizeof(float), st));
    for (int k = 0; k < 2; ++k)                // d W[ci, co, k] = sum x[ci, q] d y[co, 2q + k]
      DMEL_TRY(launch_conv_wgrad_strided(sgq.in, g, dw, C, C, 2, k, sgq.Tin, sgq.Tout, 2, k, N, st));
    DMEL_TRY(launch_conv_bgrad(g, grads + q->offset_of(pu + "0.bias"), C, N, sgq.Tout, st));
    {
      ConvRun r;
      for (int s = 0; s < 2; ++s) { r.seg[s].x = g; r.seg[s].bstride = (int64_t)C * sgq.Tout; r.seg[s].cstride = sgq.Tout; r.seg[s].Tin = sgq.Tout; }
      r.B = N; r.Tcols = sgq.Tin; r.y = other; r.y_bs = (int64_t)C * sgq.Tin; r.y_cs = sgq.Tin; r.Tout = sgq.Tin;
      DMEL_TRY(launch_conv(q->stage[j].up_dx, r, st));
    }
    std::swap(g, other);                       // g = d (stage input), length Tin
  }
  // FSQ (straight-through)
  DMEL_TRY(launch_fsq_backward(p.lat, g, q->w_in.as<float>(), q->b_in.as<float>(), q->w_out.as<float>(), other,
                               grads + q->offset_of("#fsq.w_in"), grads + q->offset_of("#fsq.b_in"), grads + q->offset_of("#fsq.w_out"),
                               grads + q->offset_of("#fsq.b_out"), p.scratch, q->fk, B, q->G, C, p.T4, st));
  std::swap(g, other);
  for (int i = q->nf - 1; i >= 0; --i) {      // downsample.{i}: Conv1d(k2, s2) -> ConvNeXtBlock
    const QStage& sgq = p.down[i];
    const std::string pd = "downsample." + std::to_string(i) + ".";
    DMEL_TRY(convnext_bwd(q->stage[i].down_cx, sgq.cx, cx_grads(*q, grads, pd + "1."), sgq.conv, g, other, N, C,
                          sgq.Tout, st));
    std::swap(g, other);                       // g = d (conv output), length Tout
    const float* xin = i == 0 ? z : sgq.in;
    float* dw = grads + q->offset_of(pd + "0.weight");
    DMEL_TRY(zero_unless_cleared(dw, (size_t)C * C * 2 * sizeof(float), st));
    for (int k = 0; k < 2; ++k)                // d W[co, ci, k] = sum d y[co, q] x[ci, 2q + k]
      DMEL_TRY(launch_conv_wgrad_strided(g, xin, dw, C, C, 2, k, sgq.Tout, sgq.Tin, 2, k, N, st));
    DMEL_TRY(launch_conv_bgrad(g, grads + q->offset_of(pd + "0.bias"), C, N, sgq.Tout, st));
    float* dst = i == 0 ? dz : other;
    if (sgq.Tin != 2 * sgq.Tout) DMEL_HIP(hipMemsetAsync(dst, 0, NC * sgq.Tin * sizeof(float), st));   // odd length: the last sample is unused
    {
      ConvRun r = run_1seg(g, C, sgq.Tout, dst, C, sgq.Tin, N);
      r.Tcols = sgq.Tout; r.out_tstride = 2; r.Tout = sgq.Tin;
      DMEL_TRY(launch_conv(q->stage[i].down_dx, r, st));
    }
    if (i > 0) std::swap(g, other);
  }
  return DMEL_OK;
}

// =====================================================================================================
// Discriminator                                     models/modules/discriminator.py:6-35
// =====================================================================================================
// Six weight-normed Conv2d over the mel image (B, 1, H = n_mels, W = frames), kernels (3, kw), stride (1, sw), SiLU in between.
// A (3, kw) Conv2d is three 1-D convolutions over W, one per kernel row dh, summed: y[:, h] += conv1d_dh(x[:, h + dh - 1]).
// Activations are kept in a flattened, zero-padded image layout (see DPlan below) in which row h + dh - 1 of the input is the same
// buffer displaced by one row pitch, so the implicit-GEMM conv kernel runs unchanged over B long items.  A stride-2 convolution
// over W is the sum of its two polyphase branches (even taps on x[2w'], odd taps on x[2w' + 1]): two K segments.
namespace {
struct DLayer {
  int Cin, Cout, kw, sw, pw;
  WeightImage fwd[3];                     // per kernel row dh
  WeightImage bwd[3][2];                  // backward-data per kernel row (and per output phase for the stride-2 layers)
  DevBuf g_dev, v_dev;                    // weight-norm parameters on the device (for d g / d v)
};
constexpr int kDiscLayers = 6;
const int kDiscCfg[kDiscLayers][5] = {{1, 64, 9, 1, 4}, {64, 128, 9, 2, 4}, {128, 256, 9, 2, 4}, {256, 512, 9, 2, 4}, {512, 1024, 3, 1, 1},
                                       {1024, 1, 3, 1, 1}};
int64_t disc_out_w(const DLayer& l, int64_t W) { return (W + 2 * l.pw - l.kw) / l.sw + 1; }
}  // namespace

struct dmel_discriminator : TrainHandle {
  DLayer layer[kDiscLayers];
};

extern "C" int dmel_discriminator_create(dmel_discriminator** out) {
  DMEL_CHECK_ARG(out, "NULL out");
  auto* d = new dmel_discriminator();
  for (int i = 0; i < kDiscLayers; ++i) {
    d->layer[i].Cin = kDiscCfg[i][0]; d->layer[i].Cout = kDiscCfg[i][1]; d->layer[i].kw = kDiscCfg[i][2]; d->layer[i].sw = kDiscCfg[i][3];
    d->layer[i].pw = kDiscCfg[i][4];
  }
  *out = d;
  return DMEL_OK;
}
extern "C" void dmel_discriminator_destroy(dmel_discriminator* d) { delete d; }
extern "C" int dmel_discriminator_set_tensor(dmel_discriminator* d, const char* key, const float* data, const int64_t* shape, int ndim) {
  return train_set_tensor(d, key, data, shape, ndim);
}

// The images of layer `p` over its folded weight W (Cout, Cin, 3, kw), one set per kernel row dh (the view's offset picks the row).
// Forward: value(row = co, ci, tap) = W[co][ci][dh][sw * tap + sg]; stride 2 is two segments, even taps on x[2w' + ...], odd taps on
// x[2w' + 1 + ...]; the bias rides the centre row's launch.
// Backward-data.  y[n] (+)= W_dh * x[n + dh - 1]  =>  d x[m] (+)= W_dh^T * d y[m - dh + 1]:
//   stride 1: the same convolution with the taps reversed (kw = 2 pw + 1, so the padding is unchanged);
//   stride 2: output phase ph of d x takes the taps dw = ph (mod 2): d x[2q + ph] = sum_t W[.., 8 - 2t - ph] d y[q + t - (2 - ph)].
static int disc_pack_layer(DLayer& l, const std::string& p, const TensorStore& ts, const float* w, bool train) {
  const int Cin = l.Cin, kw = l.kw, nseg = l.sw == 1 ? 1 : 2;
  const int64_t inner = (int64_t)Cin * 3 * kw;
  for (int dh = 0; dh < 3; ++dh) {
    PackDesc d;
    d.mode = EPI_LINEAR; d.C = l.Cout; d.nseg = nseg;
    ImageSrc src;
    for (int sg = 0; sg < nseg; ++sg) {
      d.seg[sg].Cin = Cin; d.seg[sg].taps = (kw + l.sw - 1 - sg) / l.sw; d.seg[sg].dil = 1; d.seg[sg].tstride = l.sw; d.seg[sg].toff = sg;
      d.seg[sg].pad_left = l.pw;
      ImageSeg& v = src.seg[sg];
      v.key = kFoldedWeight; v.off = dh * kw + sg; v.rs = inner; v.cs = 3 * kw; v.ts = l.sw;
    }
    if (dh == 1) src.b0 = p + "bias";
    DMEL_TRY(pack_image(l.fwd[dh], d, src, ts, w));
    for (int ph = 0; train && ph < nseg; ++ph) {
      PackDesc e;
      e.mode = EPI_LINEAR; e.C = Cin; e.nseg = 1;
      e.seg[0].Cin = l.Cout; e.seg[0].dil = 1;
      ImageSrc t;
      ImageSeg& v = t.seg[0];
      v.key = kFoldedWeight; v.rs = 3 * kw; v.cs = inner;
      if (l.sw == 1) { e.seg[0].taps = kw; e.seg[0].pad_left = l.pw; v.off = dh * kw; v.ts = 1; v.rev = 1; }
      else { e.seg[0].taps = 5 - ph; e.seg[0].pad_left = 2 - ph; v.off = dh * kw + 8 - ph; v.ts = -2; }
      DMEL_TRY(pack_image(l.bwd[dh][ph], e, t, ts, w));
    }
  }
  return DMEL_OK;
}

extern "C" int dmel_discriminator_finalize(dmel_discriminator* d) {
  DMEL_CHECK_ARG(d, "NULL handle");
  d->ready = d->train_ready = false;      // until every image is packed: a finalize that fails leaves a handle that refuses to run
  d->clear_slots();
  std::vector<float> w;                   // folded weight (Cout, Cin, 3, kw)
  for (int i = 0; i < kDiscLayers; ++i) {
    DLayer& l = d->layer[i];
    const std::string p = "blocks." + std::to_string(2 * i) + ".";
    if (!d->ts.conv_weight(p, {l.Cout, l.Cin, 3, l.kw}, w)) return DMEL_EMISSING;
    if (!d->ts.need(p + "bias", {l.Cout})) return DMEL_EMISSING;
    if (d->train) {
      const HostTensor* g0 = d->ts.need(p + "parametrizations.weight.original0", {l.Cout, 1, 1, 1});
      const HostTensor* v0 = d->ts.need(p + "parametrizations.weight.original1", {l.Cout, l.Cin, 3, l.kw});
      if (!g0 || !v0) { set_error("discriminator training needs the weight-normed form (parametrizations.weight.original0|1) of '%s'", p.c_str()); return DMEL_EMISSING; }
      DMEL_TRY(upload_vec(l.g_dev, g0->v));
      DMEL_TRY(upload_vec(l.v_dev, v0->v));
      d->add(p + "bias", l.Cout);
      d->add(p + "parametrizations.weight.original0", l.Cout);
      d->add(p + "parametrizations.weight.original1", (int64_t)l.Cout * l.Cin * 3 * l.kw);
    }
    DMEL_TRY(disc_pack_layer(l, p, d->ts, w.data(), d->train));
  }
  d->train_ready = d->train;
  d->ts.t.clear();
  d->ready = true;
  return DMEL_OK;
}

extern "C" int dmel_discriminator_set_train_precision(dmel_discriminator* d, int precision) { return train_set_precision(d, "discriminator", precision); }
extern "C" int dmel_discriminator_enable_training(dmel_discriminator* d, int on) { return train_enable(d, on); }

namespace {
// Flattened image layout.  An activation (B, C, H, W) is stored as B items of C rows of (H + 2) * P floats: image row h sits at
// [(h + 1) * P, (h + 1) * P + W), the two pad rows and the P - W gap columns of every row are zero.  With that, a kernel row dh of the
// 3 x kw convolution is a 1-D convolution over the flat axis of the same buffer displaced by (dh - 1) * P floats (horizontal taps that
// leave the image land in the zero gap, vertical ones in a zero pad row), so every launch sees 32 long items instead of B * (H + 2)
// rows of 12-94 frames and the column tiles are full.  A stride-2 layer halves the pitch: flat 2 n + dw - 4 <-> (h, 2 w + dw - 4).
// Outputs are computed on the whole flat axis; the SiLU pass that follows rewrites pads and gaps with zeros.
struct DPlan {
  float* act[kDiscLayers + 1];        // act[0]: embedded input image; act[i+1]: output of layer i (after SiLU for i < 5)
  float* pre[kDiscLayers];            // pre-activation of layer i (training keeps it; inference aliases act[i+1])
  int64_t W[kDiscLayers + 1], P[kDiscLayers + 1];     // valid width and row pitch of act[i]
  int Hp;
  int64_t guard;                      // floats in front of / behind every buffer that displaced reads may touch
  size_t bytes;
};
int64_t disc_pitch0(const dmel_discriminator* d, int64_t W) {
  for (int64_t P0 = (W + 4 + 15) / 16 * 16;; P0 += 16) {      // multiples of 16: the pitch stays even after three halvings
    int64_t w = W, P = P0;
    bool ok = true;
    for (int i = 0; i < kDiscLayers && ok; ++i) {
      const DLayer& l = d->layer[i];
      ok = P - w >= l.pw;                                   // forward taps of layer i over act[i]
      w = disc_out_w(l, w);
      if (l.sw == 2) P /= 2;
      ok = ok && P - w >= (l.sw == 2 ? 2 : l.pw);           // backward-data taps of layer i over d act[i+1]
    }
    if (ok) return P0;
  }
}
DPlan disc_plan(const dmel_discriminator* d, int B, int H, int64_t W, bool train, void* ws) {
  DPlan p{};
  Arena a(ws, (size_t)-1);
  p.Hp = H + 2;
  p.W[0] = W; p.P[0] = disc_pitch0(d, W);
  for (int i = 0; i < kDiscLayers; ++i) {
    p.W[i + 1] = disc_out_w(d->layer[i], p.W[i]);
    p.P[i + 1] = p.P[i] / d->layer[i].sw;
  }
  p.guard = p.P[0] + 64;
  auto buf = [&](int C, int64_t P) { return a.take<float>((size_t)B * C * p.Hp * P + 2 * p.guard) + p.guard; };
  p.act[0] = buf(1, p.P[0]);
  for (int i = 0; i < kDiscLayers; ++i) {
    p.act[i + 1] = buf(d->layer[i].Cout, p.P[i + 1]);
    p.pre[i] = (train && i < kDiscLayers - 1) ? buf(d->layer[i].Cout, p.P[i + 1]) : p.act[i + 1];
  }
  p.bytes = align_up(a.off, 256);
  return p;
}
__device__ __forceinline__ bool disc_valid(int col, int Hp, int P, int Wv) {
  const int h = col / P, w = col - h * P;
  return h >= 1 && h < Hp - 1 && w < Wv;
}
// grid (rows = B * C, ceil(Hp * P / 256)); y may alias u
__global__ __launch_bounds__(256) void disc_silu_fwd_kernel(const float* u, float* y, int Hp, int P, int Wv) {
  const int col = blockIdx.y * 256 + threadIdx.x, len = Hp * P;
  if (col >= len) return;
  const int64_t i = (int64_t)blockIdx.x * len + col;
  const float v = u[i];
  y[i] = disc_valid(col, Hp, P, Wv) ? v / (1.f + __expf(-v)) : 0.f;
}
// g <- g * silu'(u) on the image, 0 on pads and gaps (in place)
__global__ __launch_bounds__(256) void disc_silu_bwd_kernel(float* g, const float* __restrict__ u, int Hp, int P, int Wv) {
  const int col = blockIdx.y * 256 + threadIdx.x, len = Hp * P;
  if (col >= len) return;
  const int64_t i = (int64_t)blockIdx.x * len + col;
  const float v = u[i], sg = 1.f / (1.f + __expf(-v));
  g[i] = disc_valid(col, Hp, P, Wv) ? g[i] * sg * (1.f + v * (1.f - sg)) : 0.f;
}
// compact (B, H, Wv) -> flat (B, 1, Hp, P), zeros on pads and gaps; grid (B, ceil(Hp * P / 256))
__global__ __launch_bounds__(256) void disc_embed_kernel(const float* __restrict__ src, float* __restrict__ dst, int Hp, int P, int Wv) {
  const int col = blockIdx.y * 256 + threadIdx.x, len = Hp * P;
  if (col >= len) return;
  const int h = col / P, w = col - h * P;
  const bool ok = h >= 1 && h < Hp - 1 && w < Wv;
  dst[(int64_t)blockIdx.x * len + col] = ok ? src[((int64_t)blockIdx.x * (Hp - 2) + (h - 1)) * Wv + w] : 0.f;
}
// flat (B, 1, Hp, P) -> compact (B, H, Wv); grid (B, ceil(H * Wv / 256))
__global__ __launch_bounds__(256) void disc_extract_kernel(const float* __restrict__ src, float* __restrict__ dst, int Hp, int P, int Wv) {
  const int j = blockIdx.y * 256 + threadIdx.x, n = (Hp - 2) * Wv;
  if (j >= n) return;
  const int h = j / Wv, w = j - h * Wv;
  dst[(int64_t)blockIdx.x * n + j] = src[(int64_t)blockIdx.x * Hp * P + (int64_t)(h + 1) * P + w];
}
inline dim3 disc_grid(int64_t rows, int64_t len) { return dim3((unsigned)rows, (unsigned)((len + 255) / 256)); }

// layer i forward into `out` (pre-activation): three launches, centre row first
int disc_layer_forward(const dmel_discriminator* d, const DPlan& p, int i, int B, const float* in, float* out, hipStream_t st) {
  const DLayer& l = d->layer[i];
  const int64_t Tin = p.Hp * p.P[i], Tout = p.Hp * p.P[i + 1];
  const int order[3] = {1, 0, 2};
  for (int k = 0; k < 3; ++k) {
    const int dh = order[k];
    ConvRun r;
    const int nseg = l.sw == 1 ? 1 : 2;
    for (int sg = 0; sg < nseg; ++sg) {
      r.seg[sg].x = in + (int64_t)(dh - 1) * p.P[i]; r.seg[sg].bstride = l.Cin * Tin; r.seg[sg].cstride = Tin; r.seg[sg].Tin = Tin;
    }
    r.B = B; r.Tcols = Tout; r.y = out; r.y_bs = l.Cout * Tout; r.y_cs = Tout; r.Tout = Tout;
    r.accumulate = k > 0;
    // forward activations (log-mel images, SiLU outputs) sit in the fp16 split's range; the backward pass keeps the six-product split
    r.precision = DMEL_PRECISION_FP32_F16X2;
    DMEL_TRY(launch_conv(l.fwd[dh], r, st));
  }
  return DMEL_OK;
}
int disc_forward_common(const dmel_discriminator* d, const DPlan& p, const float* x, int B, int H, int64_t W, hipStream_t st) {
  // displaced reads run up to one row pitch past either end of an activation buffer: those guards must hold finite values
  auto zero_guards = [&](float* base, int C, int64_t P) -> hipError_t {
    hipError_t e = hipMemsetAsync(base - p.guard, 0, (size_t)p.guard * sizeof(float), st);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(base + (size_t)B * C * p.Hp * P, 0, (size_t)p.guard * sizeof(float), st);
  };
  DMEL_HIP(zero_guards(p.act[0], 1, p.P[0]));
  hipLaunchKernelGGL(disc_embed_kernel, disc_grid(B, p.Hp * p.P[0]), dim3(256), 0, st, x, p.act[0], p.Hp, (int)p.P[0], (int)W);
  DMEL_HIP(hipGetLastError());
  for (int i = 0; i < kDiscLayers; ++i) {
    const DLayer& l = d->layer[i];
    DMEL_TRY(disc_layer_forward(d, p, i, B, p.act[i], p.pre[i], st));
    if (i < kDiscLayers - 1) {
      DMEL_HIP(zero_guards(p.act[i + 1], l.Cout, p.P[i + 1]));
      hipLaunchKernelGGL(disc_silu_fwd_kernel, disc_grid((int64_t)B * l.Cout, p.Hp * p.P[i + 1]), dim3(256), 0, st, p.pre[i], p.act[i + 1], p.Hp,
                         (int)p.P[i + 1], (int)p.W[i + 1]);
      DMEL_HIP(hipGetLastError());
    }
  }
  return DMEL_OK;
}
int disc_extract(const float* flat, float* compact, int B, int Hp, int64_t P, int64_t Wv, hipStream_t st) {
  hipLaunchKernelGGL(disc_extract_kernel, disc_grid(B, (int64_t)(Hp - 2) * Wv), dim3(256), 0, st, flat, compact, Hp, (int)P, (int)Wv);
  DMEL_HIP(hipGetLastError());
  return DMEL_OK;
}
bool disc_shape_ok(const dmel_discriminator* d, int B, int H, int64_t W) {
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)B * 1024 >= ((int64_t)1 << 31)) return false;
  return (int64_t)(H + 2) * disc_pitch0(d, W) < ((int64_t)1 << 23);          // flat rows stay far inside the kernels' 32-bit offsets
}
}  // namespace

extern "C" int64_t dmel_discriminator_out_frames(const dmel_discriminator* d, int64_t W) {
  if (!d || W <= 0) return 0;
  for (int i = 0; i < kDiscLayers; ++i) W = disc_out_w(d->layer[i], W);
  return W;
}
extern "C" size_t dmel_discriminator_workspace_bytes(const dmel_discriminator* d, int B, int H, int64_t W) {
  if (!d || B <= 0 || H <= 0 || W <= 0) return 0;
  return disc_plan(d, B, H, W, false, nullptr).bytes;
}
// x (B, H, W) -> logits (B, H, W_out)           discriminator.py:34-35
extern "C" int dmel_discriminator_forward(const dmel_discriminator* d, const float* x, float* y, int B, int H, int64_t W, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(d && x && y && workspace, "discriminator_forward: NULL argument");
  if (!d->ready) { set_error("discriminator_forward: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(disc_shape_ok(d, B, H, W), "discriminator_forward: bad shape");
  const DPlan p = disc_plan(d, B, H, W, false, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= p.bytes, "discriminator_forward: workspace too small (%zu < %zu)", workspace_bytes, p.bytes);
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(disc_forward_common(d, p, x, B, H, W, st));
  return disc_extract(p.act[kDiscLayers], y, B, p.Hp, p.P[kDiscLayers], p.W[kDiscLayers], st);
}

// ---- discriminator training path -------------------------------------------------------------------------------------------
namespace {
// per output channel: d g = <dW, v> / |v|;  d v = g / |v| * (dW - v <dW, v> / |v|^2)        (torch._weight_norm, dim 0)
__global__ __launch_bounds__(256) void weight_norm_bwd_kernel(const float* __restrict__ dw, const float* __restrict__ v,
                                                              const float* __restrict__ g, float* __restrict__ dg, float* __restrict__ dv,
                                                              int64_t inner) {
  __shared__ float part[2][4];
  const int co = blockIdx.x;
  const float* dwr = dw + (int64_t)co * inner;
  const float* vr = v + (int64_t)co * inner;
  float dot = 0.f, ss = 0.f;
  for (int64_t i = threadIdx.x; i < inner; i += 256) {
    dot = fmaf(dwr[i], vr[i], dot);
    ss = fmaf(vr[i], vr[i], ss);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { dot += __shfl_xor(dot, o, 64); ss += __shfl_xor(ss, o, 64); }
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = dot; part[1][threadIdx.x >> 6] = ss; }
  __syncthreads();
  dot = part[0][0] + part[0][1] + part[0][2] + part[0][3];
  ss = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  const float nrm = sqrtf(ss), gg = g[co];
  if (threadIdx.x == 0) dg[co] = dot / nrm;
  const float k1 = gg / nrm, k2 = dot / ss;
  for (int64_t i = threadIdx.x; i < inner; i += 256) dv[(int64_t)co * inner + i] = k1 * (dwr[i] - vr[i] * k2);
}
struct DTrainPlan {
  DPlan f;
  float *ga, *gb, *dwfold;            // two gradient buffers in the flat layout (ping-pong down the layers), folded-weight gradient
  size_t bytes;
};
DTrainPlan disc_train_plan(const dmel_discriminator* d, int B, int H, int64_t W, void* ws) {
  DTrainPlan t{};
  t.f = disc_plan(d, B, H, W, true, ws);
  Arena a(ws, (size_t)-1);
  a.off = t.f.bytes;
  size_t mx = (size_t)B * t.f.Hp * t.f.P[0], mw = 0;
  for (int i = 0; i < kDiscLayers; ++i) {
    mx = std::max(mx, (size_t)B * d->layer[i].Cout * t.f.Hp * t.f.P[i + 1]);
    mw = std::max(mw, (size_t)d->layer[i].Cout * d->layer[i].Cin * 3 * d->layer[i].kw);
  }
  t.ga = a.take<float>(mx + 2 * t.f.guard) + t.f.guard;
  t.gb = a.take<float>(mx + 2 * t.f.guard) + t.f.guard;
  t.dwfold = a.take<float>(mw);
  t.bytes = align_up(a.off, 256);
  return t;
}
}  // namespace

namespace {
// folded weight on the device: W[co, :] = g[co] * v[co, :] / |v[co, :]|      (torch._weight_norm, dim 0)
__global__ __launch_bounds__(256) void weight_norm_fwd_kernel(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ w,
                                                              int64_t inner) {
  __shared__ float part[4];
  const int co = blockIdx.x;
  const float* vr = v + (int64_t)co * inner;
  float ss = 0.f;
  for (int64_t i = threadIdx.x; i < inner; i += 256) ss = fmaf(vr[i], vr[i], ss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float scale = g[co] / sqrtf(part[0] + part[1] + part[2] + part[3]);
  for (int64_t i = threadIdx.x; i < inner; i += 256) w[(int64_t)co * inner + i] = vr[i] * scale;
}
}  // namespace

// Re-pack every weight image from the device-resident bias / weight-norm g / v (after an optimiser step); `scratch` holds the folded
// weight of the largest layer (1024 * 512 * 9 floats).  (The host-side fold at finalize sums |v|^2 in double, this kernel in float:
// images agree to rounding, not bitwise.)
extern "C" int dmel_discriminator_refresh(dmel_discriminator* d, int n, const char* const* keys, const float* const* device_tensors,
                                          void* stream) {
  DMEL_CHECK_ARG(d && keys && device_tensors && n > 0, "discriminator_refresh: bad argument");
  if (!d->ready) { set_error("discriminator_refresh: handle not finalized"); return DMEL_EMISSING; }
  Refresh r("discriminator_refresh", stream);
  DMEL_TRY(r.open(n, keys, device_tensors));
  // every key is resolved before the first launch: a refused refresh leaves the handle as it was
  const float *wg[kDiscLayers], *wv[kDiscLayers];
  for (int i = 0; i < kDiscLayers; ++i) {
    const std::string p = "blocks." + std::to_string(2 * i) + ".";
    if (!r.find(p + "bias")) return DMEL_EMISSING;
    DMEL_TRY(r.need(p + "parametrizations.weight.original0", &wg[i]));
    DMEL_TRY(r.need(p + "parametrizations.weight.original1", &wv[i]));
  }
  hipStream_t st = (hipStream_t)stream;
  DevBuf& fold = *thread_scratch(2, st);
  const size_t need = (size_t)1024 * 512 * 9 * sizeof(float);
  if (fold.bytes < need) {
    fold.release();
    DMEL_HIP(hipMalloc(&fold.p, need));
    fold.bytes = need;
  }
  for (int i = 0; i < kDiscLayers; ++i) {
    DLayer& l = d->layer[i];
    const std::string p = "blocks." + std::to_string(2 * i) + ".";
    const int64_t inner = (int64_t)l.Cin * 3 * l.kw;
    float* w = fold.as<float>();
    hipLaunchKernelGGL(weight_norm_fwd_kernel, dim3((unsigned)l.Cout), dim3(256), 0, st, wv[i], wg[i], w, inner);
    DMEL_HIP(hipGetLastError());
    if (l.g_dev.p) {
      DMEL_TRY(r.copy(l.g_dev.as<float>(), p + "parametrizations.weight.original0", (size_t)l.Cout));
      DMEL_TRY(r.copy(l.v_dev.as<float>(), p + "parametrizations.weight.original1", (size_t)l.Cout * inner));
    }
    for (int dh = 0; dh < 3; ++dh) {
      DMEL_TRY(r.add(l.fwd[dh], w));
      for (int ph = 0; d->train_ready && ph < (l.sw == 1 ? 1 : 2); ++ph) DMEL_TRY(r.add(l.bwd[dh][ph], w));
    }
    DMEL_TRY(r.run());      // the 3-9 images of this layer in one launch
    // the folded weight buffer is reused by the next layer: the launches above are ordered on the same stream
  }
  return DMEL_OK;
}

extern "C" size_t dmel_discriminator_train_workspace_bytes(const dmel_discriminator* d, int B, int H, int64_t W) {
  if (!d || B <= 0 || H <= 0 || W <= 0) return 0;
  return disc_train_plan(d, B, H, W, nullptr).bytes;
}
extern "C" int64_t dmel_discriminator_grad_floats(const dmel_discriminator* d) { return train_grad_floats(d); }
extern "C" int dmel_discriminator_grad_slot(const dmel_discriminator* d, const char* key, int64_t* offset, int64_t* numel) {
  return train_grad_slot(d, "discriminator", "a parameter of the discriminator", key, offset, numel);
}

extern "C" int dmel_discriminator_forward_train(const dmel_discriminator* d, const float* x, float* y, int B, int H, int64_t W,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(d ? d->train_precision : 0);
  DMEL_CHECK_ARG(d && x && y && workspace, "discriminator_forward_train: NULL argument");
  if (!d->ready || !d->train_ready) { set_error("discriminator_forward_train: enable_training + finalize first"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(disc_shape_ok(d, B, H, W), "discriminator_forward_train: bad shape");
  const DTrainPlan t = disc_train_plan(d, B, H, W, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= t.bytes, "discriminator_forward_train: workspace too small (%zu < %zu)", workspace_bytes, t.bytes);
  hipStream_t st = (hipStream_t)stream;
  DMEL_TRY(disc_forward_common(d, t.f, x, B, H, W, st));
  return disc_extract(t.f.act[kDiscLayers], y, B, t.f.Hp, t.f.P[kDiscLayers], t.f.W[kDiscLayers], st);
}

// dy (B, H, W_out) -> dx (B, H, W) (nullable) and the parameter gradients (bias, weight-norm g and v of every layer) in `grads`
extern "C" int dmel_discriminator_backward(const dmel_discriminator* d, const float* dy, float* dx, float* grads, int B, int H, int64_t W,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  TrainPrecisionScope train_scope(d ? d->train_precision : 0);
  DMEL_CHECK_ARG(d && dy && grads && workspace, "discriminator_backward: NULL argument");
  if (!d->ready || !d->train_ready) { set_error("discriminator_backward: enable_training + finalize first"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(disc_shape_ok(d, B, H, W), "discriminator_backward: bad shape");
  const DTrainPlan t = disc_train_plan(d, B, H, W, workspace);
  DMEL_CHECK_ARG(workspace_bytes >= t.bytes, "discriminator_backward: workspace too small (%zu < %zu)", workspace_bytes, t.bytes);
  hipStream_t st = (hipStream_t)stream;
  const DPlan& p = t.f;
  const int Hp = p.Hp;
  // gradients live in the flat layout of the activation they belong to.  Their guards are only ever multiplied into pad / gap outputs,
  // which the SiLU backward pass rewrites with zeros, but they are cleared once so that every read is of defined memory.
  DMEL_HIP(hipMemsetAsync(t.ga - p.guard, 0, (size_t)p.guard * sizeof(float), st));
  DMEL_HIP(hipMemsetAsync(t.gb - p.guard, 0, (size_t)p.guard * sizeof(float), st));
  float* g = t.ga;
  hipLaunchKernelGGL(disc_embed_kernel, disc_grid(B, Hp * p.P[kDiscLayers]), dim3(256), 0, st, dy, g, Hp, (int)p.P[kDiscLayers],
                     (int)p.W[kDiscLayers]);
  DMEL_HIP(hipGetLastError());
  bool g_is_a = true;
  for (int i = kDiscLayers - 1; i >= 0; --i) {
    const DLayer& l = d->layer[i];
    const std::string pk = "blocks." + std::to_string(2 * i) + ".";
    const int64_t Tin = Hp * p.P[i], Tout = Hp * p.P[i + 1];
    // g: d act[i+1] (B, Cout, Hp * P).  Through the SiLU (not after the last layer), in place, zero on pads and gaps.
    if (i < kDiscLayers - 1) {
      hipLaunchKernelGGL(disc_silu_bwd_kernel, disc_grid((int64_t)B * l.Cout, Tout), dim3(256), 0, st, g, p.pre[i], Hp, (int)p.P[i + 1],
                         (int)p.W[i + 1]);
      DMEL_HIP(hipGetLastError());
    }
    // bias and weight gradients: one launch per kernel row, the kw horizontal taps on the grid.  The fp16-split kernels that read g (the
    // weight gradients and, below, backward-data) scale it by its max, found once per layer.
    DMEL_TRY(launch_conv_bgrad(g, grads + d->offset_of(pk + "bias"), l.Cout, B, Tout, st));
    DMEL_HIP(hipMemsetAsync(t.dwfold, 0, (size_t)l.Cout * l.Cin * 3 * l.kw * sizeof(float), st));
    const uint32_t* g_absmax = nullptr;
    DMEL_TRY(launch_absmax(g, (int64_t)B * l.Cout * Tout, st, &g_absmax));
    for (int dh = 0; dh < 3; ++dh)
      DMEL_TRY(launch_conv_wgrad_strided(g, p.act[i] + (int64_t)(dh - 1) * p.P[i], t.dwfold, l.Cout, l.Cin, l.sw, -l.pw, Tout, Tin, 3 * l.kw,
                                         dh * l.kw, B, st, l.kw, g_absmax));
    hipLaunchKernelGGL(weight_norm_bwd_kernel, dim3((unsigned)l.Cout), dim3(256), 0, st, t.dwfold, l.v_dev.as<float>(), l.g_dev.as<float>(),
                       grads + d->offset_of(pk + "parametrizations.weight.original0"),
                       grads + d->offset_of(pk + "parametrizations.weight.original1"), (int64_t)l.Cin * 3 * l.kw);
    DMEL_HIP(hipGetLastError());
    if (i == 0 && !dx) break;
    // backward-data into the other buffer (B, Cin, Hp * P[i])
    float* dst = g_is_a ? t.gb : t.ga;
    const int order[3] = {1, 0, 2};
    for (int k = 0; k < 3; ++k) {
      const int dh = order[k];
      const int nph = l.sw == 1 ? 1 : 2;
      for (int ph = 0; ph < nph; ++ph) {
        ConvRun r = run_1seg(g - (int64_t)(dh - 1) * p.P[i + 1], l.Cout, Tout, dst, l.Cin, Tin, B);
        r.accumulate = k > 0;
        if (g_absmax) { r.precision = DMEL_PRECISION_FP32_F16X2; r.seg[0].in_absmax = g_absmax; }
        if (l.sw == 2) {
          r.out_tstride = 2; r.phase_base = ph; r.Tcols = Tin / 2; r.Tout = Tin;
        }
        DMEL_TRY(launch_conv(l.bwd[dh][ph], r, st));
      }
    }
    g = dst;
    g_is_a = !g_is_a;
  }
  if (dx) DMEL_TRY(disc_extract(g, dx, B, Hp, p.P[0], W, st));      // layer 0 has no SiLU in front: its pads / gaps are simply not read
  return DMEL_OK;
}

// =====================================================================================================
// BigVGAN                                          models/modules/bigvgan/bigvgan.py:244-407
// =====================================================================================================
namespace {
struct SnakeP {
  DevBuf alpha, beta;
};
struct AmpBlock {             // AMPBlock1, bigvgan.py:31-147
  int k;
  int dil[3];
  PackedConv c1[3], c2[3];
  PackedConv c1T[3], c2T[3];  // backward-data images (transposed, tap-reversed), packed by dmel_bigvgan_enable_input_grad
  SnakeP act[6];
};
struct UpStage {
  int u, k, Cin, Cout;
  PackedConv lo, hi;          // phases [0,u/2) with taps d={-1,0}; phases [u/2,u) with taps d={0,+1}
  bool one = false;           // u = 2, 4, 8: the stage can run as one launch of `all`
  // every phase in one image, rows phase-minor (m = co u + ph), taps d={-1,0,+1}.  Packed on the FIRST forward that wants it
  // (ensure_up_stage_all), from the weights the two images above hold exactly -- like the backward-data images, not at finalize
  mutable PackedConv all;
  mutable bool all_ready = false;
  std::vector<PackedConv> dgrad;   // backward-data: u/2 images of two strided two-tap segments each (pack_up_stage_dgrad); empty until asked for
};
// ConvTranspose1d(Cin, Cout, k = 2u, stride u, padding u/2) as two groups of u/2 phase sub-convolutions with two taps each:
//   y[co, u q + ph] = sum_ci sum_d W[ci, co, ph + u/2 - u d] x[ci, q + d]                    (bigvgan.py:320-334, :371-374)
// w: (Cin, Cout, k) host floats, bias: Cout host floats.  us.u / k / Cin / Cout are set by the caller.
int pack_up_stage(UpStage& us, const float* w, const float* bias) {
  const int u = us.u, k = us.k, hu = u / 2, Co = us.Cout;
  for (int half = 0; half < 2; ++half) {
    PackDesc d;
    d.mode = EPI_LINEAR; d.nseg = 1; d.C = Co; d.phases = hu;
    d.seg[0].Cin = us.Cin; d.seg[0].taps = 2; d.seg[0].dil = 1; d.seg[0].pad_left = half == 0 ? 1 : 0;
    DMEL_TRY(pack_conv(half == 0 ? us.lo : us.hi, d,
                       [&](int, int row, int ci, int tap) {
                         const int ph = row / Co + half * hu, co = row % Co;
                         const int dd = tap - (half == 0 ? 1 : 0);
                         const int kk = ph + hu - u * dd;
                         return (kk >= 0 && kk < k) ? w[((size_t)ci * Co + co) * k + kk] : 0.f;
                       },
                       [&](int row) { return bias ? bias[row % Co] : 0.f; }));
  }
  us.one = u == 2 || u == 4 || u == 8;
  us.all_ready = false;       // new weights: the one-launch image is re-packed by the next forward
  return DMEL_OK;
}
// One image for the whole stage (u = 2, 4, 8): the union of the two tap windows, d = {-1, 0, +1} behind pad_left = 1, over all u phases.
// The tap a phase does not use (d = +1 below u/2, d = -1 from u/2 on) falls outside [0, k) and carries zero weights: a K step that adds
// zero products leaves an fp32 accumulator as it was, and the two real taps keep their order (chunk-major, d ascending), so every output
// keeps the bits of the two launches.  Rows are phase-minor, m = co u + ph: a lane of the 32 x 32 accumulator tile then holds
// consecutive output samples of one channel in consecutive registers (conv_dev.h, epi_phase_tile), and x is read once per stage.
int pack_up_stage_all(const UpStage& us, const float* w, const float* bias) {
  const int u = us.u, k = us.k, hu = u / 2, Co = us.Cout;
  PackDesc d;
  d.mode = EPI_LINEAR; d.nseg = 1; d.C = Co * u; d.phases = 1; d.row_u = u; d.dead_taps = 1;
  d.seg[0].Cin = us.Cin; d.seg[0].taps = 3; d.seg[0].dil = 1; d.seg[0].pad_left = 1;
  return pack_conv(us.all, d,
                   [&](int, int row, int ci, int tap) {
                     const int co = row / u, ph = row % u, kk = ph + hu - u * (tap - 1);
                     return (kk >= 0 && kk < k) ? w[((size_t)ci * Co + co) * k + kk] : 0.f;
                   },
                   [&](int row) { return bias[row / u]; });
}
int ensure_up_stage_all(const UpStage& us);
// DMEL_UPSTAGE_ONE_LAUNCH=0: every transposed convolution runs as the two phase-major launches (A/B, bit-identity tests).  Read per call.
static bool upstage_one_launch_enabled() {
  const char* e = getenv("DMEL_UPSTAGE_ONE_LAUNCH");
  return !(e && e[0] == '0' && e[1] == 0);
}
// x (B, Cin, T) -> y (B, Cout, u T).  in_len (nullable, B device int64): item b's valid input columns; what lies behind them reads as zero
int launch_up_stage(const UpStage& us, const float* x, float* y, int B, int64_t T, int precision, hipStream_t st,
                    const int64_t* in_len = nullptr) {
  if (us.one && upstage_one_launch_enabled()) {
    DMEL_TRY(ensure_up_stage_all(us));
    ConvRun r = run_1seg(x, us.Cin, T, y, us.Cout, T * us.u, B);
    r.seg[0].in_len = in_len;
    r.Tcols = T; r.Tout = T * us.u;
    r.precision = precision;
    return launch_conv(us.all, r, st);
  }
  for (int half = 0; half < 2; ++half) {
    ConvRun r = run_1seg(x, us.Cin, T, y, us.Cout, T * us.u, B);
    r.seg[0].in_len = in_len;
    r.Tcols = T; r.out_tstride = us.u; r.phase_base = half * (us.u / 2); r.Tout = T * us.u;
    r.precision = precision;
    DMEL_TRY(launch_conv(half == 0 ? us.lo : us.hi, r, st));
  }
  return DMEL_OK;
}
// Host copy of a packed fp32 weight image, and the value at (packed row m, K step, reduction row k of the step): the inverse of the
// layout pack_conv writes (conv.h).  The backward-data images are packed from it after finalize has dropped the state dict; the fp32
// image holds the folded weights exactly.
struct HostImage {
  std::vector<float> w;
  int steps = 0;
  int load(const PackedConv& pc) {
    steps = pc.steps;
    w.resize(pc.w.bytes / sizeof(float));
    if (!w.empty()) DMEL_HIP(hipMemcpy(w.data(), pc.w.p, pc.w.bytes, hipMemcpyDeviceToHost));
    return DMEL_OK;
  }
  float at(int m, int step, int k) const {
    const int tile = m >> 5, r = m & 31, h = k & 1, kk = k >> 1, hf = kk >> 2, j = kk & 3;
    return w[((((size_t)tile * steps + step) * 2 + hf) * 64 + 32 * h + r) * 4 + j];
  }
};
// W[co][ci][tap] of a "same" convolution packed by pack_same_conv (one segment, identity row map)
float same_conv_weight(const HostImage& im, int taps, int co, int ci, int tap) { return im.at(co, (ci / kCK) * taps + tap, ci % kCK); }
// (Cin, Cout, k) weights of a transposed convolution back from the forward images of pack_up_stage: the one-launch image once a forward
// has packed it (row co u + ph, three taps per chunk), else the two phase-major ones
int unpack_up_stage(const UpStage& us, std::vector<float>& w) {
  const int u = us.u, k = us.k, hu = u / 2, Co = us.Cout;
  w.assign((size_t)us.Cin * Co * k, 0.f);
  if (us.all_ready) {
    HostImage im;
    DMEL_TRY(im.load(us.all));
    for (int co = 0; co < Co; ++co)
      for (int ph = 0; ph < u; ++ph)
        for (int ci = 0; ci < us.Cin; ++ci)
          for (int tap = 0; tap < 3; ++tap) {
            const int kk = ph + hu - u * (tap - 1);
            if (kk >= 0 && kk < k) w[((size_t)ci * Co + co) * k + kk] = im.at(co * u + ph, (ci / kCK) * 3 + tap, ci % kCK);
          }
    return DMEL_OK;
  }
  for (int half = 0; half < 2; ++half) {
    const PackedConv& pc = half == 0 ? us.lo : us.hi;
    HostImage im;
    DMEL_TRY(im.load(pc));
    for (int p = 0; p < hu; ++p)
      for (int co = 0; co < Co; ++co)
        for (int ci = 0; ci < us.Cin; ++ci)
          for (int tap = 0; tap < 2; ++tap) {
            const int ph = p + half * hu, dd = tap - (half == 0 ? 1 : 0), kk = ph + hu - u * dd;
            if (kk >= 0 && kk < k) w[((size_t)ci * Co + co) * k + kk] = im.at(p * pc.RP + co, (ci / kCK) * 2 + tap, ci % kCK);
          }
  }
  return DMEL_OK;
}
// The one-launch image of a stage, packed by the first forward that wants it: weights and bias are read back from the phase-major images
// (the fp32 image and the bias rows hold them exactly; finalize has dropped the state dict).  That call copies between host and device
// and synchronises, so it must not be the first thing a stream capture records: run one forward before capturing, as the streaming
// decoder does.  One lock for all stages: lanes and sessions share a vocoder handle between threads.
int ensure_up_stage_all(const UpStage& us) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (us.all_ready) return DMEL_OK;
  std::vector<float> w, bias(us.lo.bias.bytes / sizeof(float));
  DMEL_TRY(unpack_up_stage(us, w));
  if (!bias.empty()) DMEL_HIP(hipMemcpy(bias.data(), us.lo.bias.p, us.lo.bias.bytes, hipMemcpyDeviceToHost));      // rows [0, Cout): phase 0
  DMEL_CHECK_ARG((int)bias.size() >= us.Cout, "conv_transpose1d: the phase-major bias image is shorter than Cout");
  DMEL_TRY(pack_up_stage_all(us, w.data(), bias.data()));
  us.all_ready = true;
  return DMEL_OK;
}
// Backward-data of the transposed convolution:  dx[ci, q] = scale * sum_co sum_kk W[ci, co, kk] dy[co, u q + kk - u/2]  (zero outside
// dy) -- a stride-u, 2u-tap convolution of dy.  Tap kk = u m + ph (m = 0, 1; ph < u) reads dy[u (q + m) + ph - u/2]: phase ph is one
// strided segment of the implicit-GEMM kernel (SegDesc::tstride = u, toff = ph, pad_left = u/2, two taps that step by u).  A launch
// carries two segments, so the u phases are u/2 launches, the later ones accumulating into dx (the small tensor of the pair).
// scale: the vocoder folds the 1 / num_kernels of the stage's block average in here.
int pack_up_stage_dgrad(UpStage& us, const float* w, float scale) {
  const int u = us.u, k = us.k, Co = us.Cout;
  us.dgrad.clear();
  us.dgrad.resize(u / 2);
  for (int j = 0; j < u / 2; ++j) {
    PackDesc d;
    d.mode = EPI_LINEAR; d.nseg = 2; d.C = us.Cin; d.phases = 1;
    for (int sg = 0; sg < 2; ++sg) {
      d.seg[sg].Cin = Co; d.seg[sg].taps = 2; d.seg[sg].dil = 1; d.seg[sg].tstride = u; d.seg[sg].toff = 2 * j + sg; d.seg[sg].pad_left = u / 2;
    }
    DMEL_TRY(pack_conv(us.dgrad[j], d,
                       [&](int sg, int row /*ci*/, int cc /*co*/, int tap) { return scale * w[((size_t)row * Co + cc) * k + u * tap + 2 * j + sg]; },
                       [&](int) { return 0.f; }));
  }
  return DMEL_OK;
}
// dy (B, Cout, u T) -> dx (B, Cin, T); six-product split (a gradient tensor is the operand)
int launch_up_stage_dgrad(const UpStage& us, const float* dy, float* dx, int B, int64_t T, hipStream_t st) {
  const int64_t Tu = T * us.u;
  for (size_t j = 0; j < us.dgrad.size(); ++j) {
    ConvRun r = run_1seg(dy, us.Cout, Tu, dx, us.Cin, T, B);
    r.seg[1] = r.seg[0];
    r.accumulate = j > 0;
    r.precision = DMEL_PRECISION_FP32;
    DMEL_TRY(launch_conv(us.dgrad[j], r, st));
  }
  return DMEL_OK;
}
}  // namespace

// ---- standalone transposed convolution / output convolution (C-ABI rows convT1d, conv_post of SURVEY section 8(b)) ---------------
struct dmel_conv_transpose {
  UpStage us;
  int precision = 0;
  std::vector<float> w_host;      // kept for the lazily packed backward-data images
};
extern "C" int dmel_conv_transpose1d_create(dmel_conv_transpose** out, const float* w_host, const float* bias_host, int Cin, int Cout, int k,
                                            int stride) {
  DMEL_CHECK_ARG(out && w_host, "conv_transpose1d_create: NULL argument");
  DMEL_CHECK_ARG(Cin > 0 && Cout > 0 && stride >= 2 && (stride % 2) == 0, "conv_transpose1d_create: bad shape (even stride >= 2 required)");
  if (k != 2 * stride) {
    set_error("conv_transpose1d: only k == 2 * stride with padding stride / 2 (every BigVGAN up-sampler) is built, got k %d stride %d", k, stride);
    return DMEL_EUNSUPPORTED;
  }
  auto* h = new dmel_conv_transpose();
  h->us.u = stride; h->us.k = k; h->us.Cin = Cin; h->us.Cout = Cout;
  const int rc = pack_up_stage(h->us, w_host, bias_host);
  if (rc != DMEL_OK) { delete h; return rc; }
  h->w_host.assign(w_host, w_host + (size_t)Cin * Cout * k);
  *out = h;
  return DMEL_OK;
}
extern "C" int dmel_conv_transpose1d_backward_data(dmel_conv_transpose* h, const float* dy, float* dx, int B, int64_t T, void* stream) {
  DMEL_CHECK_ARG(h && dy && dx, "conv_transpose1d_backward_data: NULL argument");
  DMEL_CHECK_ARG(B > 0 && T > 0, "conv_transpose1d_backward_data: bad shape");
  if (h->us.dgrad.empty()) DMEL_TRY(pack_up_stage_dgrad(h->us, h->w_host.data(), 1.f));
  return launch_up_stage_dgrad(h->us, dy, dx, B, T, (hipStream_t)stream);
}
extern "C" int dmel_conv_post_backward_f32(const float* y, const float* dy, const float* w_dev, int act, float* dx, int B, int C, int K,
                                           int64_t T, void* stream) {
  DMEL_CHECK_ARG(dy && w_dev && dx && (y || act == 0), "conv_post_backward: NULL argument");
  DMEL_CHECK_ARG(act == 0 || act == 2 || act == 3, "conv_post_backward: act must be 0 (none), 2 (tanh) or 3 (clamp to [-1, 1])");
  return launch_conv_post_bwd(y, dy, dx, w_dev, act == 0 ? ACT_NONE : act == 2 ? ACT_TANH : ACT_CLAMP1, B, C, K, T, (hipStream_t)stream);
}
extern "C" void dmel_conv_transpose1d_destroy(dmel_conv_transpose* h) { delete h; }
extern "C" int dmel_conv_transpose1d_set_precision(dmel_conv_transpose* h, int precision) {
  DMEL_CHECK_ARG(h && valid_precision(precision), "conv_transpose1d_set_precision: not a DMEL_PRECISION_* value");
  h->precision = precision;
  return DMEL_OK;
}
extern "C" int dmel_conv_transpose1d_forward(const dmel_conv_transpose* h, const float* x, float* y, int B, int64_t T, void* stream) {
  DMEL_CHECK_ARG(h && x && y, "conv_transpose1d_forward: NULL argument");
  DMEL_CHECK_ARG(B > 0 && T > 0, "conv_transpose1d_forward: bad shape");
  return launch_up_stage(h->us, x, y, B, T, h->precision, (hipStream_t)stream);
}
extern "C" int dmel_conv_transpose1d_forward_items(const dmel_conv_transpose* h, const float* x, float* y, int B, int64_t T,
                                                   const int64_t* lengths_dev, void* stream) {
  DMEL_CHECK_ARG(h && x && y && lengths_dev, "conv_transpose1d_forward_items: NULL argument");
  DMEL_CHECK_ARG(B > 0 && T > 0, "conv_transpose1d_forward_items: bad shape");
  return launch_up_stage(h->us, x, y, B, T, h->precision, (hipStream_t)stream, lengths_dev);
}
extern "C" int dmel_conv_post_f32(const float* x, const float* w_dev, float bias, int act, float* y, int B, int C, int K, int64_t T, void* stream) {
  DMEL_CHECK_ARG(x && w_dev && y, "conv_post: NULL argument");
  DMEL_CHECK_ARG(act == 0 || act == 2 || act == 3, "conv_post: act must be 0 (none), 2 (tanh) or 3 (clamp to [-1, 1])");
  return launch_conv_post(x, y, w_dev, bias, act == 0 ? ACT_NONE : act == 2 ? ACT_TANH : ACT_CLAMP1, B, C, K, T, (hipStream_t)stream);
}

extern "C" int dmel_conv_post_items_f32(const float* x, const float* w_dev, float bias, int act, float* y, int B, int C, int K, int64_t T,
                                        const int64_t* lengths_dev, void* stream) {
  DMEL_CHECK_ARG(x && w_dev && y && lengths_dev, "conv_post_items: NULL argument");
  DMEL_CHECK_ARG(act == 0 || act == 2 || act == 3, "conv_post_items: act must be 0 (none), 2 (tanh) or 3 (clamp to [-1, 1])");
  return launch_conv_post(x, y, w_dev, bias, act == 0 ? ACT_NONE : act == 2 ? ACT_TANH : ACT_CLAMP1, B, C, K, T, (hipStream_t)stream, lengths_dev);
}

struct dmel_bigvgan {
  dmel_bigvgan_config cfg;
  TensorStore ts;
  bool ready = false;
  PackedConv conv_pre;
  DevBuf post_w;            // conv_post weight (1, C, 7) on the device: a single output row runs as a reduction kernel
  float post_bias = 0.f;
  int post_c = 0;
  std::vector<UpStage> ups;
  std::vector<AmpBlock> blocks;
  SnakeP act_post;
  float taps_up[12], taps_dn[12];   // UpSample1d.filter / DownSample1d.lowpass.filter (the reference registers the same 12 taps for both)
  int64_t total_up = 1;
  // The AMP blocks of a stage are independent until their outputs are averaged: they run on the caller's stream plus
  // up to two library-owned side streams, forked and joined with events around every stage, so the VALU-bound
  // anti-alias activations of one block overlap the MFMA-bound convolutions of another.  Semantics on the caller's
  // stream are unchanged (everything is ordered behind what was on it and finished when the final join is reached).
  static constexpr int kSide = 2;
  hipStream_t side[kSide] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[kSide] = {nullptr, nullptr}, ev_chain[3] = {nullptr, nullptr, nullptr},
             ev_stag[3] = {nullptr, nullptr, nullptr};
  bool multi = false;
  int precision = 0;
  PackedConv conv_preT;     // backward-data image of conv_pre
  bool input_grad = false;  // the backward-data images are packed (dmel_bigvgan_enable_input_grad)
  ~dmel_bigvgan() {
    for (int i = 0; i < kSide; ++i) {
      if (side[i]) (void)hipStreamDestroy(side[i]);
      if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
    }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (auto& e : ev_chain) if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_stag) if (e) (void)hipEventDestroy(e);
  }
};

extern "C" int dmel_bigvgan_create(dmel_bigvgan** out, const dmel_bigvgan_config* cfg) {
  DMEL_CHECK_ARG(out && cfg, "NULL argument");
  DMEL_CHECK_ARG(cfg->num_upsamples >= 1 && cfg->num_upsamples <= 8 && cfg->num_kernels >= 1 && cfg->num_kernels <= 8,
                 "bigvgan: bad stage/kernel count");
  DMEL_CHECK_ARG(cfg->num_mels > 0 && cfg->upsample_initial_channel > 0, "bigvgan: bad channel counts");
  DMEL_CHECK_ARG(cfg->resblock_type >= 0 && cfg->resblock_type <= 2, "bigvgan: resblock_type must be 1 (AMPBlock1) or 2 (AMPBlock2)");
  int64_t up = 1;
  for (int i = 0; i < cfg->num_upsamples; ++i) {
    const int u = cfg->upsample_rates[i], k = cfg->upsample_kernel_sizes[i];
    if (k != 2 * u || (u % 2) != 0) {
      set_error("bigvgan: upsample stage %d (rate %d, kernel %d) unsupported: kernel must be 2*rate with an even rate", i, u, k);
      return DMEL_EUNSUPPORTED;
    }
    DMEL_CHECK_ARG((cfg->upsample_initial_channel >> (i + 1)) > 0, "bigvgan: channel count underflows at stage %d", i);
    up *= u;
  }
  for (int j = 0; j < cfg->num_kernels; ++j) {
    DMEL_CHECK_ARG(cfg->resblock_kernel_sizes[j] % 2 == 1, "bigvgan: even resblock kernel");
    for (int l = 0; l < 3; ++l)
      if ((cfg->resblock_kernel_sizes[j] - 1) * cfg->resblock_dilations[j][l] > 64) {
        set_error("bigvgan: resblock kernel %d dilation %d exceeds the 64-sample halo", cfg->resblock_kernel_sizes[j],
                  cfg->resblock_dilations[j][l]);
        return DMEL_EUNSUPPORTED;
      }
  }
  auto* m = new dmel_bigvgan();
  m->cfg = *cfg;
  m->total_up = up;
  // kaiser_sinc_filter1d(0.25, 0.3, 12) as the reference computes it in fp32 (filter.py:30-62); overridden by any
  // "*.filter" buffer found in the state dict.
  static const float kTaps[12] = {0.0020289647f, 0.0093894657f, -0.0255434588f, -0.0576573834f, 0.1285725832f, 0.4432097971f,
                                  0.4432097971f, 0.1285725832f, -0.0576573834f, -0.0255434588f, 0.0093894657f, 0.0020289647f};
  std::memcpy(m->taps_up, kTaps, sizeof(kTaps));
  std::memcpy(m->taps_dn, kTaps, sizeof(kTaps));
  *out = m;
  return DMEL_OK;
}
extern "C" void dmel_bigvgan_destroy(dmel_bigvgan* m) { delete m; }
extern "C" int dmel_bigvgan_set_precision(dmel_bigvgan* m, int precision) {
  DMEL_CHECK_ARG(m && valid_precision(precision), "bigvgan_set_precision: not a DMEL_PRECISION_* value");
  m->precision = precision;
  return DMEL_OK;
}
extern "C" int dmel_bigvgan_set_tensor(dmel_bigvgan* m, const char* key, const float* data, const int64_t* shape, int ndim) {
  DMEL_CHECK_ARG(m, "NULL handle");
  m->ready = false;
  return m->ts.set(key, data, shape, ndim);
}

static int pack_same_conv(PackedConv& pc, const TensorStore& ts, const std::string& prefix, int Cout, int Cin, int k, int dil,
                          bool has_bias) {
  std::vector<float> w;
  if (!ts.conv_weight(prefix, {Cout, Cin, k}, w)) return DMEL_EMISSING;
  const HostTensor* b = nullptr;
  if (has_bias) {
    b = ts.need(prefix + "bias", {Cout});
    if (!b) return DMEL_EMISSING;
  }
  PackDesc d;
  d.mode = EPI_LINEAR; d.nseg = 1; d.C = Cout;
  d.seg[0].Cin = Cin; d.seg[0].taps = k; d.seg[0].dil = dil; d.seg[0].pad_left = dil * (k - 1) / 2;  // get_padding, utils.py:57-58
  return pack_conv(pc, d, [&](int, int row, int ci, int tap) { return w[((size_t)row * Cin + ci) * k + tap]; },
                   [&](int row) { return b ? b->v[row] : 0.f; });
}

static int load_snake(SnakeP& s, const TensorStore& ts, const std::string& prefix, int C, bool snake) {
  const HostTensor* a = ts.need(prefix + "act.alpha", {C});
  if (!a) return DMEL_EMISSING;
  DMEL_TRY(upload_vec(s.alpha, a->v));
  if (!snake) {
    const HostTensor* b = ts.need(prefix + "act.beta", {C});
    if (!b) return DMEL_EMISSING;
    DMEL_TRY(upload_vec(s.beta, b->v));
  }
  return DMEL_OK;
}

extern "C" int dmel_bigvgan_finalize(dmel_bigvgan* m) {
  DMEL_CHECK_ARG(m, "NULL handle");
  const dmel_bigvgan_config& c = m->cfg;
  const bool snake = c.activation_snake != 0;
  // anti-alias taps: every Activation1d registers two buffers ("...upsample.filter", "...downsample.lowpass.filter"); all up filters
  // must agree with each other and all down filters with each other (one launch-constant pair per model); up and down may differ
  bool have_up = false, have_dn = false;
  for (auto& kv : m->ts.t) {
    const std::string& k = kv.first;
    const bool is_f = k.size() > 7 && k.compare(k.size() - 7, 7, ".filter") == 0;
    if (!is_f) continue;
    if (kv.second.numel() != 12) { set_error("bigvgan: filter '%s' is not 12 taps", k.c_str()); return DMEL_EUNSUPPORTED; }
    const bool is_dn = k.find("downsample") != std::string::npos;
    float* dst = is_dn ? m->taps_dn : m->taps_up;
    bool& have = is_dn ? have_dn : have_up;
    if (!have) { std::memcpy(dst, kv.second.v.data(), 12 * sizeof(float)); have = true; }
    else if (std::memcmp(dst, kv.second.v.data(), 12 * sizeof(float)) != 0) {
      set_error("bigvgan: anti-alias filter '%s' differs from the other %s filters (per-activation filters unsupported)", k.c_str(),
                is_dn ? "down-sampling" : "up-sampling");
      return DMEL_EUNSUPPORTED;
    }
  }
  const int C0 = c.upsample_initial_channel;
  DMEL_TRY(pack_same_conv(m->conv_pre, m->ts, "conv_pre.", C0, c.num_mels, 7, 1, true));
  m->ups.clear(); m->blocks.clear();
  m->ups.resize(c.num_upsamples);
  m->blocks.resize((size_t)c.num_upsamples * c.num_kernels);
  int ch = C0;
  for (int i = 0; i < c.num_upsamples; ++i) {
    UpStage& us = m->ups[i];
    us.u = c.upsample_rates[i]; us.k = c.upsample_kernel_sizes[i]; us.Cin = C0 >> i; us.Cout = C0 >> (i + 1);
    ch = us.Cout;
    const std::string p = "ups." + std::to_string(i) + ".0.";
    std::vector<float> w;  // ConvTranspose1d weight (Cin, Cout, k)
    if (!m->ts.conv_weight(p, {us.Cin, us.Cout, us.k}, w)) return DMEL_EMISSING;
    const HostTensor* b = m->ts.need(p + "bias", {us.Cout});
    if (!b) return DMEL_EMISSING;
    DMEL_TRY(pack_up_stage(us, w.data(), b->v.data()));
    for (int j = 0; j < c.num_kernels; ++j) {
      AmpBlock& ab = m->blocks[(size_t)i * c.num_kernels + j];
      ab.k = c.resblock_kernel_sizes[j];
      const std::string bp = "resblocks." + std::to_string(i * c.num_kernels + j) + ".";
      for (int l = 0; l < 3; ++l) {
        ab.dil[l] = c.resblock_dilations[j][l];
        if (c.resblock_type == 2) {   // AMPBlock2: one dilated conv per layer (bigvgan.py:176-191), three activations
          DMEL_TRY(pack_same_conv(ab.c1[l], m->ts, bp + "convs." + std::to_string(l) + ".", ch, ch, ab.k, ab.dil[l], true));
        } else {
          DMEL_TRY(pack_same_conv(ab.c1[l], m->ts, bp + "convs1." + std::to_string(l) + ".", ch, ch, ab.k, ab.dil[l], true));
          DMEL_TRY(pack_same_conv(ab.c2[l], m->ts, bp + "convs2." + std::to_string(l) + ".", ch, ch, ab.k, 1, true));
        }
      }
      for (int a = 0; a < (c.resblock_type == 2 ? 3 : 6); ++a)
        DMEL_TRY(load_snake(ab.act[a], m->ts, bp + "activations." + std::to_string(a) + ".", ch, snake));
    }
  }
  if (!m->ev_fork) {
    m->multi = c.num_kernels <= 3 && c.num_kernels > 1;
    DMEL_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < 3; ++i) DMEL_HIP(hipEventCreateWithFlags(&m->ev_chain[i], hipEventDisableTiming));
    for (int i = 0; i < 3; ++i) DMEL_HIP(hipEventCreateWithFlags(&m->ev_stag[i], hipEventDisableTiming));
    for (int i = 0; i < dmel_bigvgan::kSide; ++i) {
      DMEL_HIP(hipStreamCreateWithFlags(&m->side[i], hipStreamNonBlocking));
      DMEL_HIP(hipEventCreateWithFlags(&m->ev_join[i], hipEventDisableTiming));
    }
  }
  DMEL_TRY(load_snake(m->act_post, m->ts, "activation_post.", ch, snake));
  {
    std::vector<float> pw;
    if (!m->ts.conv_weight("conv_post.", {1, ch, 7}, pw)) return DMEL_EMISSING;
    m->post_bias = 0.f;
    if (c.use_bias_at_final) {
      const HostTensor* pb = m->ts.need("conv_post.bias", {1});
      if (!pb) return DMEL_EMISSING;
      m->post_bias = pb->v[0];
    }
    DMEL_TRY(upload_vec(m->post_w, pw));
    m->post_c = ch;
  }
  m->ts.t.clear();
  m->ready = true;
  m->input_grad = false;    // the images belong to the previous weights
  m->conv_preT = PackedConv();
  return DMEL_OK;
}

constexpr int kBigvganBufs = 12;   // x, xu, xs + 3 x (xj, ua, vb)
extern "C" int dmel_bigvgan_set_streams(dmel_bigvgan* m, int n_streams) {
  DMEL_CHECK_ARG(m, "NULL handle");
  DMEL_CHECK_ARG(n_streams == 1 || n_streams == 3, "bigvgan: 1 or 3 streams supported");
  m->multi = n_streams == 3 && m->cfg.num_kernels > 1 && m->cfg.num_kernels <= 3 && m->ev_fork != nullptr;
  return DMEL_OK;
}

static size_t bigvgan_plan(const dmel_bigvgan* m, int B, int64_t T, void* ws, float* bufs[kBigvganBufs]) {
  const dmel_bigvgan_config& c = m->cfg;
  size_t mx = (size_t)c.upsample_initial_channel * T;
  int64_t Tc = T;
  for (int i = 0; i < c.num_upsamples; ++i) {
    Tc *= c.upsample_rates[i];
    mx = std::max(mx, (size_t)(c.upsample_initial_channel >> (i + 1)) * Tc);
  }
  Arena a(ws, (size_t)-1);
  for (int i = 0; i < kBigvganBufs; ++i) {
    float* p = a.take<float>(mx * B);
    if (bufs) bufs[i] = p;
  }
  return align_up(a.off, 256);
}

extern "C" size_t dmel_bigvgan_workspace_bytes(const dmel_bigvgan* m, int B, int64_t T) {
  if (!m || B <= 0 || T <= 0) return 0;
  return bigvgan_plan(m, B, T, nullptr, nullptr);
}

// The per-stage length tables of the items form live behind the buffers of the plain plan: (num_upsamples + 1) x B int64.
static size_t bigvgan_items_plan(const dmel_bigvgan* m, int B, int64_t T, void* ws, float* bufs[kBigvganBufs], int64_t** tabs) {
  const size_t off = bigvgan_plan(m, B, T, ws, bufs);
  if (tabs) *tabs = reinterpret_cast<int64_t*>(static_cast<char*>(ws) + off);
  return align_up(off + (size_t)(m->cfg.num_upsamples + 1) * B * sizeof(int64_t), 256);
}

extern "C" size_t dmel_bigvgan_items_workspace_bytes(const dmel_bigvgan* m, int B, int64_t T) {
  if (!m || B <= 0 || T <= 0) return 0;
  return bigvgan_items_plan(m, B, T, nullptr, nullptr, nullptr);
}

// lengths == nullptr: dmel_bigvgan_forward.  Otherwise dmel_bigvgan_forward_items: the same launches, each told its stage's lengths.
static int bigvgan_forward_impl(const dmel_bigvgan* m, const float* mel, const int64_t* lengths, float* audio, int B, int64_t T,
                                void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = lengths ? "bigvgan_forward_items" : "bigvgan_forward";
  DMEL_CHECK_ARG(m && mel && audio && workspace, "%s: NULL argument", who);
  if (!m->ready) { set_error("%s: handle not finalized", who); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(B > 0 && T > 0, "%s: bad shape", who);
  float* bufs[kBigvganBufs];
  int64_t* tab = nullptr;
  const size_t need = lengths ? bigvgan_items_plan(m, B, T, workspace, bufs, &tab) : bigvgan_plan(m, B, T, workspace, bufs);
  DMEL_CHECK_ARG(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const dmel_bigvgan_config& c = m->cfg;
  // Items: table i holds every item's length at stage i (lengths[b] * prod(upsample_rates[:i]), clamped into the pitch), and ONE
  // invariant holds from conv_pre to conv_post: columns at or beyond an item's length hold garbage, and NOTHING READS THEM -- every
  // convolution's staging turns them into its zero padding (SegRun::in_len), the activations and conv_post take the item forms, and the
  // epilogues (bias, residual, running sum, 1 / out_div) are column-wise.  So columns [0, length) of an item are, launch by launch, the
  // bits of a batch of one at T = length, whatever its batch peers hold.
  if (lengths) {
    LenScales sc;
    sc.v[0] = 1;
    for (int i = 0; i < c.num_upsamples; ++i) sc.v[i + 1] = sc.v[i] * c.upsample_rates[i];
    DMEL_TRY(launch_length_tables(lengths, tab, B, T, c.num_upsamples + 1, sc, st));
  }
  auto len_at = [&](int stage) -> const int64_t* { return lengths ? tab + (size_t)stage * B : nullptr; };
  auto act = [&](const float* in, float* out, const SnakeP& p, int ch_, int64_t Tc_, const int64_t* len, hipStream_t s_) {
    if (len) return launch_aa_snake_items(in, out, p.alpha.as<float>(), p.beta.as<float>(), m->taps_up, m->taps_dn, c.snake_logscale, B, ch_, Tc_, len, s_);
    return launch_aa_snake(in, out, p.alpha.as<float>(), p.beta.as<float>(), m->taps_up, m->taps_dn, c.snake_logscale, B, ch_, Tc_, s_);
  };
  // "fp32-grade, library's choice": nothing downstream of the vocoder is discrete, so its default is the three-product fp16 split
  // (include/dmel_hip.h); DMEL_PRECISION_FP32_BF16X3 asks for the six-product bf16 split
  const int prec = m->precision == DMEL_PRECISION_FP32 ? DMEL_PRECISION_FP32_F16X2 : m->precision;
  const int logscale = c.snake_logscale;
  float *x = bufs[0], *xu = bufs[1], *xs = bufs[2];
  float* ua = bufs[4];   // block 0's activation scratch doubles as the post-activation buffer

  {  // conv_pre (bigvgan.py:369)
    ConvRun r = run_1seg(mel, c.num_mels, T, x, c.upsample_initial_channel, T, B);
    r.seg[0].in_len = len_at(0);
    r.precision = prec;
    DMEL_TRY(launch_conv(m->conv_pre, r, st));
  }
  int64_t Tc = T;
  int ch = c.upsample_initial_channel;
  for (int i = 0; i < c.num_upsamples; ++i) {
    const UpStage& us = m->ups[i];
    const int64_t Tn = Tc * us.u;
    DMEL_TRY(launch_up_stage(us, x, xu, B, Tc, prec, st, len_at(i)));  // transposed conv as two phase groups (bigvgan.py:371-374)
    ch = us.Cout;
    Tc = Tn;
    const int64_t bs = (int64_t)ch * Tc;
    const bool multi = m->multi;
    const int64_t* len = len_at(i + 1);
    if (multi) {  // fork: the side streams start behind the transposed conv
      DMEL_HIP(hipEventRecord(m->ev_fork, st));
      for (int k = 0; k < dmel_bigvgan::kSide; ++k) DMEL_HIP(hipStreamWaitEvent(m->side[k], m->ev_fork, 0));
    }
    // The three blocks each begin with an activation of the SAME tensor xu: on one stream they are one launch (aa_snake3_kernel reads and
    // up-filters xu once) into the three blocks' activation buffers, and each block's l == 0 activation is skipped.  DMEL_SNAKE_HEAD3=0
    // keeps the three launches (same bits; read per call, for A/B and the equality tests).  The multi-stream form keeps them too: there
    // the heads are what the stagger events hang on.
    const char* fuse_env = getenv("DMEL_FUSE_SNAKE");
    const bool fuse = fuse_env && fuse_env[0] == '1' && !lengths;
    const char* head_env = getenv("DMEL_SNAKE_HEAD3");
    const bool head3 = !multi && !fuse && c.num_kernels == 3 && !(head_env && head_env[0] == '0');
    if (head3) {
      float* const hy[3] = {bufs[4], bufs[7], bufs[10]};
      const float *ha[3], *hb[3];
      for (int j = 0; j < 3; ++j) {
        const SnakeP& p = m->blocks[(size_t)i * 3 + j].act[0];
        ha[j] = p.alpha.as<float>();
        hb[j] = p.beta.as<float>();
      }
      DMEL_TRY(launch_aa_snake3(xu, hy, ha, hb, m->taps_up, m->taps_dn, logscale, B, ch, Tc, len, st));
    }
    for (int j = 0; j < c.num_kernels; ++j) {  // AMPBlock1.forward (bigvgan.py:132-141), summed and averaged (:376-382)
      const AmpBlock& ab = m->blocks[(size_t)i * c.num_kernels + j];
      hipStream_t sj = (multi && j > 0) ? m->side[j - 1] : st;
      float *xj = bufs[3 + 3 * j], *uj = bufs[4 + 3 * j], *vj = bufs[5 + 3 * j];
      const float* xin = xu;
      // DMEL_FUSE_SNAKE=1: every act -> conv pair as ONE kernel (conv_snake.hip: producer waves compute the activation, consumer waves run
      // the MFMA loop).  Bit-identical to the two-kernel form and measured SLOWER on every vocoder shape (0.54-1.03x,
      // profiles/r03_fused_vs_two_kernels.txt; DESIGN.md section 4 has the probes that explain it), so the two-kernel form stays the
      // default.  Read per call so that a test can flip it inside one process.  The fused kernel has one row length for the whole batch:
      // it stands aside for items.
      for (int l = 0; l < 3; ++l) {
        // stagger the branches by one kernel: started together they run snake|snake|snake then conv|conv|conv in lockstep
        // and the VALU-bound activations never meet the matrix-pipe-bound convolutions on a CU
        if (l == 0 && multi && j > 0) DMEL_HIP(hipStreamWaitEvent(sj, m->ev_stag[j - 1], 0));
        if (c.resblock_type == 2) {   // AMPBlock2.forward (bigvgan.py:232-237): xt = a(x); xt = c(xt); x = xt + x
          ConvRun r2 = run_1seg(uj, ch, Tc, l < 2 ? xj : xs, ch, Tc, B);
          r2.seg[0].in_len = len;
          r2.res = xin; r2.res_bs = bs; r2.res_cs = Tc;
          r2.precision = prec;
          const bool fuse2 = fuse && conv_snake_eligible(ab.c1[l], r2);
          if (!fuse2 && !(head3 && l == 0)) DMEL_TRY(act(xin, uj, ab.act[l], ch, Tc, len, sj));
          if (!fuse2 && l == 0 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_stag[j], sj));
          if (l == 2) {
            r2.accumulate = j > 0;
            if (j == c.num_kernels - 1) r2.out_div = (float)c.num_kernels;
            if (multi && j > 0) DMEL_HIP(hipStreamWaitEvent(sj, m->ev_chain[j - 1], 0));
          }
          if (fuse2) {
            r2.seg[0].x = xin;
            DMEL_TRY(launch_conv_snake(ab.c1[l], r2, ab.act[l].alpha.as<float>(), ab.act[l].beta.as<float>(), m->taps_up, m->taps_dn, logscale, sj));
            if (l == 0 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_stag[j], sj));
          } else {
            DMEL_TRY(launch_conv(ab.c1[l], r2, sj));
          }
          if (l == 2 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_chain[j], sj));
          xin = xj;
          continue;
        }
        ConvRun r1 = run_1seg(uj, ch, Tc, vj, ch, Tc, B);
        r1.seg[0].in_len = len;
        r1.precision = prec;
        if (fuse && conv_snake_eligible(ab.c1[l], r1)) {       // act -> conv as ONE kernel: the activated tensor never exists in HBM
          r1.seg[0].x = xin;
          DMEL_TRY(launch_conv_snake(ab.c1[l], r1, ab.act[2 * l].alpha.as<float>(), ab.act[2 * l].beta.as<float>(), m->taps_up, m->taps_dn, logscale, sj));
          if (l == 0 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_stag[j], sj));
        } else {
          if (!(head3 && l == 0)) DMEL_TRY(act(xin, uj, ab.act[2 * l], ch, Tc, len, sj));
          if (l == 0 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_stag[j], sj));
          DMEL_TRY(launch_conv(ab.c1[l], r1, sj));
        }
        ConvRun r2 = run_1seg(uj, ch, Tc, l < 2 ? xj : xs, ch, Tc, B);
        r2.seg[0].in_len = len;
        r2.res = xin; r2.res_bs = bs; r2.res_cs = Tc;
        r2.precision = prec;
        const bool fuse2 = fuse && conv_snake_eligible(ab.c2[l], r2);
        if (!fuse2) DMEL_TRY(act(vj, uj, ab.act[2 * l + 1], ch, Tc, len, sj));
        if (l == 2) {
          // xs = ((out_0 + out_1) + out_2) / 3, in the reference's order: block j's last conv runs behind block j-1's
          r2.accumulate = j > 0;
          if (j == c.num_kernels - 1) r2.out_div = (float)c.num_kernels;
          if (multi && j > 0) DMEL_HIP(hipStreamWaitEvent(sj, m->ev_chain[j - 1], 0));
        }
        if (fuse2) {
          r2.seg[0].x = vj;
          DMEL_TRY(launch_conv_snake(ab.c2[l], r2, ab.act[2 * l + 1].alpha.as<float>(), ab.act[2 * l + 1].beta.as<float>(), m->taps_up, m->taps_dn, logscale, sj));
        } else {
          DMEL_TRY(launch_conv(ab.c2[l], r2, sj));
        }
        if (l == 2 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_chain[j], sj));
        xin = xj;
      }
    }
    if (multi) {  // join: the caller's stream continues behind every side stream
      for (int k = 0; k < dmel_bigvgan::kSide && k + 1 < c.num_kernels; ++k) {
        DMEL_HIP(hipEventRecord(m->ev_join[k], m->side[k]));
        DMEL_HIP(hipStreamWaitEvent(st, m->ev_join[k], 0));
      }
    }
    std::swap(x, xs);
  }
  // activation_post, conv_post, tanh | clamp (bigvgan.py:385-391)
  const int64_t* len_out = len_at(c.num_upsamples);
  // one launch: the activated tensor goes through LDS, not HBM (snake_post_kernel).  DMEL_POST_FUSED=0 keeps the two launches (same bits).
  const char* post_env = getenv("DMEL_POST_FUSED");
  if (!(post_env && post_env[0] == '0'))
    return launch_snake_post(x, audio, m->act_post.alpha.as<float>(), m->act_post.beta.as<float>(), m->taps_up, m->taps_dn, logscale,
                             m->post_w.as<float>(), m->post_bias, c.use_tanh_at_final ? ACT_TANH : ACT_CLAMP1, B, ch, 7, Tc, len_out, st);
  DMEL_TRY(act(x, ua, m->act_post, ch, Tc, len_out, st));
  return launch_conv_post(ua, audio, m->post_w.as<float>(), m->post_bias, c.use_tanh_at_final ? ACT_TANH : ACT_CLAMP1, B, ch, 7,
                          Tc, st, len_out);
}

extern "C" int dmel_bigvgan_forward(const dmel_bigvgan* m, const float* mel, float* audio, int B, int64_t T, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return bigvgan_forward_impl(m, mel, nullptr, audio, B, T, workspace, workspace_bytes, stream);
}

extern "C" int dmel_bigvgan_forward_items(const dmel_bigvgan* m, const float* mel, const int64_t* lengths_dev, float* audio, int B, int64_t T,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(lengths_dev, "bigvgan_forward_items: NULL lengths");
  return bigvgan_forward_impl(m, mel, lengths_dev, audio, B, T, workspace, workspace_bytes, stream);
}

// ---- input gradient through the frozen generator (bigvgan.py:367-393 under autograd, weights frozen as in codec_lit_modules.py:68-72) ----
extern "C" int dmel_bigvgan_enable_input_grad(dmel_bigvgan* m, int on) {
  DMEL_CHECK_ARG(m, "bigvgan_enable_input_grad: NULL handle");
  if (!m->ready) { set_error("bigvgan_enable_input_grad: handle not finalized"); return DMEL_EMISSING; }
  const dmel_bigvgan_config& c = m->cfg;
  if (!on) {
    m->input_grad = false;
    m->conv_preT = PackedConv();
    for (auto& us : m->ups) us.dgrad.clear();
    for (auto& ab : m->blocks)
      for (int l = 0; l < 3; ++l) { ab.c1T[l] = PackedConv(); ab.c2T[l] = PackedConv(); }
    return DMEL_OK;
  }
  if (m->input_grad) return DMEL_OK;
  // dx = conv1d(dy, W transposed and tap-reversed): the image dmel_conv_backward_data packs, from the forward image's own values
  auto pack_T = [](PackedConv& dst, const PackedConv& fwd, int Cout, int Cin, int k, int dil) -> int {
    HostImage im;
    DMEL_TRY(im.load(fwd));
    PackDesc d;
    d.mode = EPI_LINEAR; d.nseg = 1; d.C = Cin; d.phases = 1;
    d.seg[0].Cin = Cout; d.seg[0].taps = k; d.seg[0].dil = dil; d.seg[0].pad_left = dil * (k - 1) / 2;
    return pack_conv(dst, d, [&](int, int row /*ci*/, int cc /*co*/, int tap) { return same_conv_weight(im, k, cc, row, k - 1 - tap); },
                     [&](int) { return 0.f; });
  };
  DMEL_TRY(pack_T(m->conv_preT, m->conv_pre, c.upsample_initial_channel, c.num_mels, 7, 1));
  for (int i = 0; i < c.num_upsamples; ++i) {
    UpStage& us = m->ups[i];
    std::vector<float> w;
    DMEL_TRY(unpack_up_stage(us, w));
    DMEL_TRY(pack_up_stage_dgrad(us, w.data(), 1.f / (float)c.num_kernels));   // the block average of the stage rides on these weights
    for (int j = 0; j < c.num_kernels; ++j) {
      AmpBlock& ab = m->blocks[(size_t)i * c.num_kernels + j];
      for (int l = 0; l < 3; ++l) {
        DMEL_TRY(pack_T(ab.c1T[l], ab.c1[l], us.Cout, us.Cout, ab.k, ab.dil[l]));
        if (c.resblock_type != 2) DMEL_TRY(pack_T(ab.c2T[l], ab.c2[l], us.Cout, us.Cout, ab.k, 1));
      }
    }
  }
  m->input_grad = true;
  return DMEL_OK;
}

namespace {
// Workspace of forward_train / backward_input.  Saved for the backward (untouched between the two calls): the audio, per stage the
// up-sampled tensor and per AMP block the x of layers 1, 2 and (AMPBlock1) the three conv1 outputs -- 16 slots per stage with three
// blocks -- and the input of activation_post (the last of the two ping-pong stage buffers).  Scratch: one activation buffer per block
// for the forward; two gradient ping-pong buffers, the stage's input gradient and four buffers per block for the backward.
struct BvTrainPlan {
  float* audio;
  float* ping[2];
  float* ua[8];
  struct Stage { float* xu; float* xl[8][3]; float* v[8][3]; } st[8];
  float *G[2], *D;
  float* blk[8][4];
  size_t bytes;
};
size_t bigvgan_train_plan(const dmel_bigvgan* m, int B, int64_t T, void* ws, BvTrainPlan* p) {
  const dmel_bigvgan_config& c = m->cfg;
  BvTrainPlan local;
  BvTrainPlan& q = p ? *p : local;
  Arena a(ws, (size_t)-1);
  size_t mx = (size_t)std::max(c.upsample_initial_channel, c.num_mels) * T;
  int64_t Tc = T;
  q.audio = a.take<float>((size_t)B * T * m->total_up);
  for (int i = 0; i < c.num_upsamples; ++i) {
    Tc *= c.upsample_rates[i];
    const size_t n = (size_t)(c.upsample_initial_channel >> (i + 1)) * Tc;
    mx = std::max(mx, n);
    q.st[i].xu = a.take<float>(n * B);
    for (int j = 0; j < c.num_kernels; ++j)
      for (int l = 0; l < 3; ++l) {
        q.st[i].xl[j][l] = l > 0 ? a.take<float>(n * B) : q.st[i].xu;
        q.st[i].v[j][l] = c.resblock_type == 2 ? nullptr : a.take<float>(n * B);
      }
  }
  for (int k = 0; k < 2; ++k) q.ping[k] = a.take<float>(mx * B);
  for (int j = 0; j < c.num_kernels; ++j) q.ua[j] = a.take<float>(mx * B);
  for (int k = 0; k < 2; ++k) q.G[k] = a.take<float>(mx * B);
  q.D = a.take<float>(mx * B);
  for (int j = 0; j < c.num_kernels; ++j)
    for (int k = 0; k < 4; ++k) q.blk[j][k] = a.take<float>(mx * B);
  q.bytes = align_up(a.off, 256);
  return q.bytes;
}
}  // namespace

extern "C" size_t dmel_bigvgan_train_workspace_bytes(const dmel_bigvgan* m, int B, int64_t T) {
  if (!m || B <= 0 || T <= 0) return 0;
  return bigvgan_train_plan(m, B, T, nullptr, nullptr);
}

// dmel_bigvgan_forward with the input of every activation kept: the same launches with the same arguments on other buffers (always the
// two-kernel act -> conv form), so the audio is bit-identical to dmel_bigvgan_forward's.
extern "C" int dmel_bigvgan_forward_train(const dmel_bigvgan* m, const float* mel, float* audio, int B, int64_t T, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(m && mel && audio && workspace, "bigvgan_forward_train: NULL argument");
  DMEL_CHECK_ARG(m->input_grad, "bigvgan_forward_train: dmel_bigvgan_enable_input_grad(m, 1) has not been called on this handle");
  if (!m->ready) { set_error("bigvgan_forward_train: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(B > 0 && T > 0, "bigvgan_forward_train: bad shape");
  BvTrainPlan p;
  const size_t need = bigvgan_train_plan(m, B, T, workspace, &p);
  DMEL_CHECK_ARG(workspace_bytes >= need, "bigvgan_forward_train: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const dmel_bigvgan_config& c = m->cfg;
  const int prec = m->precision == DMEL_PRECISION_FP32 ? DMEL_PRECISION_FP32_F16X2 : m->precision;
  const int logscale = c.snake_logscale;
  const bool multi = m->multi;
  float* x = p.ping[0];
  {  // conv_pre (bigvgan.py:369)
    ConvRun r = run_1seg(mel, c.num_mels, T, x, c.upsample_initial_channel, T, B);
    r.precision = prec;
    DMEL_TRY(launch_conv(m->conv_pre, r, st));
  }
  int64_t Tc = T;
  int ch = c.upsample_initial_channel;
  for (int i = 0; i < c.num_upsamples; ++i) {
    const UpStage& us = m->ups[i];
    float* xu = p.st[i].xu;
    float* xs = p.ping[(i + 1) & 1];
    DMEL_TRY(launch_up_stage(us, x, xu, B, Tc, prec, st));
    ch = us.Cout;
    Tc *= us.u;
    const int64_t bs = (int64_t)ch * Tc;
    if (multi) {
      DMEL_HIP(hipEventRecord(m->ev_fork, st));
      for (int k = 0; k < dmel_bigvgan::kSide; ++k) DMEL_HIP(hipStreamWaitEvent(m->side[k], m->ev_fork, 0));
    }
    for (int j = 0; j < c.num_kernels; ++j) {
      const AmpBlock& ab = m->blocks[(size_t)i * c.num_kernels + j];
      hipStream_t sj = (multi && j > 0) ? m->side[j - 1] : st;
      float* uj = p.ua[j];
      for (int l = 0; l < 3; ++l) {
        const float* xin = p.st[i].xl[j][l];
        float* xout = l < 2 ? p.st[i].xl[j][l + 1] : xs;
        if (l == 0 && multi && j > 0) DMEL_HIP(hipStreamWaitEvent(sj, m->ev_stag[j - 1], 0));
        const bool two = c.resblock_type != 2;
        const SnakeP& a1 = ab.act[two ? 2 * l : l];
        DMEL_TRY(launch_aa_snake(xin, uj, a1.alpha.as<float>(), a1.beta.as<float>(), m->taps_up, m->taps_dn, logscale, B, ch, Tc, sj));
        if (l == 0 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_stag[j], sj));
        if (two) {
          float* vj = p.st[i].v[j][l];
          ConvRun r1 = run_1seg(uj, ch, Tc, vj, ch, Tc, B);
          r1.precision = prec;
          DMEL_TRY(launch_conv(ab.c1[l], r1, sj));
          const SnakeP& a2 = ab.act[2 * l + 1];
          DMEL_TRY(launch_aa_snake(vj, uj, a2.alpha.as<float>(), a2.beta.as<float>(), m->taps_up, m->taps_dn, logscale, B, ch, Tc, sj));
        }
        ConvRun r2 = run_1seg(uj, ch, Tc, xout, ch, Tc, B);
        r2.res = xin; r2.res_bs = bs; r2.res_cs = Tc;
        r2.precision = prec;
        if (l == 2) {  // xs = ((out_0 + out_1) + out_2) / num_kernels in the reference's order, as in dmel_bigvgan_forward
          r2.accumulate = j > 0;
          if (j == c.num_kernels - 1) r2.out_div = (float)c.num_kernels;
          if (multi && j > 0) DMEL_HIP(hipStreamWaitEvent(sj, m->ev_chain[j - 1], 0));
        }
        DMEL_TRY(launch_conv(two ? ab.c2[l] : ab.c1[l], r2, sj));
        if (l == 2 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_chain[j], sj));
      }
    }
    if (multi) {
      for (int k = 0; k < dmel_bigvgan::kSide && k + 1 < c.num_kernels; ++k) {
        DMEL_HIP(hipEventRecord(m->ev_join[k], m->side[k]));
        DMEL_HIP(hipStreamWaitEvent(st, m->ev_join[k], 0));
      }
    }
    x = xs;
  }
  float* ua = p.ua[0];
  DMEL_TRY(launch_aa_snake(x, ua, m->act_post.alpha.as<float>(), m->act_post.beta.as<float>(), m->taps_up, m->taps_dn, logscale, B, ch, Tc, st));
  DMEL_TRY(launch_conv_post(ua, audio, m->post_w.as<float>(), m->post_bias, c.use_tanh_at_final ? ACT_TANH : ACT_CLAMP1, B, ch, 7, Tc, st));
  DMEL_HIP(hipMemcpyAsync(p.audio, audio, (size_t)B * Tc * sizeof(float), hipMemcpyDeviceToDevice, st));   // act' of conv_post needs it
  return DMEL_OK;
}

// The forward in reverse: conv_post', activation_post', per stage the AMP blocks and the transposed conv's backward-data, conv_pre's
// backward-data.  Inside a block the gradient is carried UNSCALED (the block is linear in it); the blocks' input gradients are summed
// in block order by the store of each block's last activation backward (dx = (dx_act + residual) + running sum: one stream and three
// give equal bits), and the 1 / num_kernels of the average sits in the transposed conv's backward-data weights.  No add / scale launch.
extern "C" int dmel_bigvgan_backward_input(const dmel_bigvgan* m, const float* daudio, float* dmel, int B, int64_t T, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  DMEL_CHECK_ARG(m && daudio && dmel && workspace, "bigvgan_backward_input: NULL argument");
  DMEL_CHECK_ARG(m->input_grad, "bigvgan_backward_input: dmel_bigvgan_enable_input_grad(m, 1) has not been called on this handle");
  if (!m->ready) { set_error("bigvgan_backward_input: handle not finalized"); return DMEL_EMISSING; }
  DMEL_CHECK_ARG(B > 0 && T > 0, "bigvgan_backward_input: bad shape");
  BvTrainPlan p;
  const size_t need = bigvgan_train_plan(m, B, T, workspace, &p);
  DMEL_CHECK_ARG(workspace_bytes >= need, "bigvgan_backward_input: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const dmel_bigvgan_config& c = m->cfg;
  const int logscale = c.snake_logscale;
  const bool multi = m->multi;
  const bool two = c.resblock_type != 2;
  const int nu = c.num_upsamples;
  int ch = c.upsample_initial_channel >> nu;
  int64_t Tc = T * m->total_up;
  auto snake_bwd = [&](const SnakeP& a, const float* xin, const float* dy, float* dx, const float* radd, const float* racc, int C,
                       int64_t Tn, hipStream_t s) {
    return launch_aa_snake_bwd_input(xin, dy, dx, radd, racc, a.alpha.as<float>(), a.beta.as<float>(), m->taps_up, m->taps_dn, logscale, B,
                                     C, Tn, s);
  };
  auto dgrad = [&](const PackedConv& pc, const float* dy, float* dx, int C, int64_t Tn, hipStream_t s) {
    ConvRun r = run_1seg(dy, C, Tn, dx, C, Tn, B);
    r.precision = DMEL_PRECISION_FP32;      // six-product split: the operand is a gradient tensor as it is
    return launch_conv(pc, r, s);
  };
  float* g = p.G[0];
  {  // conv_post' (with the derivative of tanh | clamp from the saved audio), activation_post'
    float* dua = p.blk[0][0];
    DMEL_TRY(launch_conv_post_bwd(p.audio, daudio, dua, m->post_w.as<float>(), c.use_tanh_at_final ? ACT_TANH : ACT_CLAMP1, B, ch, 7, Tc, st));
    DMEL_TRY(snake_bwd(m->act_post, p.ping[nu & 1], dua, g, nullptr, nullptr, ch, Tc, st));
  }
  for (int i = nu - 1; i >= 0; --i) {
    const UpStage& us = m->ups[i];
    ch = us.Cout;
    if (multi) {
      DMEL_HIP(hipEventRecord(m->ev_fork, st));
      for (int k = 0; k < dmel_bigvgan::kSide; ++k) DMEL_HIP(hipStreamWaitEvent(m->side[k], m->ev_fork, 0));
    }
    for (int j = 0; j < c.num_kernels; ++j) {
      const AmpBlock& ab = m->blocks[(size_t)i * c.num_kernels + j];
      hipStream_t sj = (multi && j > 0) ? m->side[j - 1] : st;
      float *t1 = p.blk[j][2], *t2 = p.blk[j][3];
      const float* gx = g;                  // gradient of x_{l+1}; the stage's output gradient for the last layer
      for (int l = 2; l >= 0; --l) {
        const float* xin = p.st[i].xl[j][l];
        float* gout = l > 0 ? p.blk[j][l - 1] : p.D;
        // layer l: x_{l+1} = c2(a2(c1(a1(x_l)))) + x_l   (AMPBlock2: x_{l+1} = c(a(x_l)) + x_l)
        if (two) {
          DMEL_TRY(dgrad(ab.c2T[l], gx, t1, ch, Tc, sj));
          DMEL_TRY(snake_bwd(ab.act[2 * l + 1], p.st[i].v[j][l], t1, t2, nullptr, nullptr, ch, Tc, sj));
          DMEL_TRY(dgrad(ab.c1T[l], t2, t1, ch, Tc, sj));
        } else {
          DMEL_TRY(dgrad(ab.c1T[l], gx, t1, ch, Tc, sj));
        }
        const float* racc = nullptr;
        if (l == 0 && j > 0) {              // D = ((d_0 + d_1) + d_2): block j's last store runs behind block j-1's
          racc = p.D;
          if (multi) DMEL_HIP(hipStreamWaitEvent(sj, m->ev_chain[j - 1], 0));
        }
        DMEL_TRY(snake_bwd(ab.act[two ? 2 * l : l], xin, t1, gout, gx, racc, ch, Tc, sj));
        if (l == 0 && multi && j + 1 < c.num_kernels) DMEL_HIP(hipEventRecord(m->ev_chain[j], sj));
        gx = gout;
      }
    }
    if (multi) {
      for (int k = 0; k < dmel_bigvgan::kSide && k + 1 < c.num_kernels; ++k) {
        DMEL_HIP(hipEventRecord(m->ev_join[k], m->side[k]));
        DMEL_HIP(hipStreamWaitEvent(st, m->ev_join[k], 0));
      }
    }
    Tc /= us.u;
    float* gn = g == p.G[0] ? p.G[1] : p.G[0];
    DMEL_TRY(launch_up_stage_dgrad(us, p.D, gn, B, Tc, st));   // carries the 1 / num_kernels
    g = gn;
  }
  {  // conv_pre backward-data
    ConvRun r = run_1seg(g, c.upsample_initial_channel, T, dmel, c.num_mels, T, B);
    r.precision = DMEL_PRECISION_FP32;
    DMEL_TRY(launch_conv(m->conv_preT, r, st));
  }
  return DMEL_OK;
}
