// The options of rdgan_set_option (include/rdgan.h documents what each one does): the fields, and ONE table row per option with its
// name, how a caller's value is normalised, which cached weight forms it shapes, and its default.  Host-only and free of HIP: a plain
// C++ compiler builds this header on its own (tests/test_options_host.py does).
//
// The rule: an option that shapes cached forms says so in its table row.  gen_build_forms / prep_critic_weights (rdgan_api.hip)
// compare rd_form_key() of the flagged rows with the key the forms in the workspace were built under, so flag every option either
// builder reads, directly or through a predicate -- an unflagged one leaves stale weight images under rdgan_set_weight_versions.
#pragma once
#include <limits.h>
#include <string.h>

// every integer rdgan_set_option writes, and nothing else (rdgan_handle inherits these: h->collapse, h->a16, ...)
struct RdOptions {
  // 1: 8-tap collapsed generator blocks (default); 0: direct 27-tap form
  int collapse = 1;
  // 1: producer/consumer (wave-specialised, LDS-DMA) kernel for the big clean GEMMs; 2: also for small problems (tests)
  int wave_spec = 1;
  // 1: bf16 storage mode (option "bf16"; needs the collapsed + shared-centre forms)
  int a16 = 0;
  // 1: backward of the 64 -> 1 conv straight from the dlogits (no im2col matrix), fused with block 3's PixelNorm backward
  int g9_direct = 1;
  // 1: forward of generator blocks 2, 3 as shared part T = S x + difference part (48 instead of 64 tap products); -1: by storage mode
  int fast_fwd = -1;
  // 1: generator blocks' weight/input gradients in the shared-centre form along d (48 instead of 64 tap products); -1: by storage mode
  int fast_bwd = -1;
  // 1: last generator conv sums its in-tile taps in the GEMM epilogue; 0: full column matrix + gather kernel
  int tapgather = 1;
  // 1: bf16 forward GEMMs of the shared-centre form keep the tile's source rows resident in LDS (k_conv_gemm_ws<..., RES>)
  int resident = 1;
  // 1: bf16 storage mode, ndomain 16: block 3 forward (collapsed form) by the slab kernel k_upconv_slab16
  int upconv_slab = 1;
  // 1: bf16 storage mode, source planes larger than 8 x 8 (ndomain 32, 64, ...: multiples of 16): block 3 forward by k_upconv_slab_t16
  int upconv_slab_t = 1;
  // 1: the same for block 2 (k_upconv2_slab16)
  int upconv2_slab = 1;
  // 1: with the block-3 slab kernel, the last conv's tap products come out of that kernel's epilogue (no pass over h3; critic steps
  // do not store h3 at all)
  int g9_fused = 1;
  // 1: bf16 storage mode, ndomain 16: layer-1 forward / second sweep with a sample resident in LDS (k_d1_fwd_sample16)
  int d1_fwd_sample = 1;
  // 1: bf16 storage mode: input gradient of the last conv + block 3's PixelNorm backward on the fp32 matrix pipe (k_g9_bwd_mfma16)
  int g9_bwd_mfma = 1;
  // 1: bf16 storage mode: the generator's Dense layer on the bf16 matrix pipe (inputs and kernel rounded to bf16, K padded to 64)
  int dense16 = 1;
  // 1: ... and, on a handle of max_batch <= 128, by k_dense16_skinny (weights and inputs streamed in fragment order, no LDS)
  int dense_skinny = 1;
  // 1: the weight gradients of critic layers 2-4 (streaming kernels) on the border-class boxes too
  int wgrad_boxes = 1;
  // 1: forward / second-sweep GEMMs of critic layers 2-4 skip the taps that leave the picture (plan_conv_fwd_boxes); 2: at every size (tests)
  int border_boxes = 1;
  // 1: bf16 storage mode, ndomain 16: weight gradient of critic layer 3 by k_d3_wgrad_slab16
  int d3_wgrad_slab = 1;
  // 1: bf16 storage mode, ndomain 16: weight gradient of critic layer 2 by k_d2_wgrad_slab16
  int d2_wgrad_slab = 1;
  // 1: bf16 storage mode, ndomain 16, collapsed form: weight gradient of generator block 3 by k_upconv_wgrad_slab16
  int upwgrad_slab = 1;
  // 1: ndomain 16: dD/d(sample) of layer 1 in one pass per sample (k_d1_dgrad_sample16; fp32 storage: k_d1_dgrad_sample32, which in
  // the critic step also takes the penalty's norm pass k_gp_norm_r0)
  int d1_dgrad_fused = 1;
  // 1: fp32 storage, shared-centre backward: the next PixelNorm backward folds the difference part's gradient into dx itself (no k_combine_dx)
  int combine_dx_fused = 1;
  // 1: bf16 storage mode: layer-1 weight gradient + bias gradient on the bf16 matrix pipe (k_d1_wgrad16)
  int d1_wgrad16 = 1;
  // 1: bf16 weight gradients of N % 128 == 0 layers with >= 32768 rows on 256 x 128 tiles, three stages (k_wgrad_gemm_ws16<256,128>):
  // measured SLOWER, default off
  int wgrad_wide = 0;
  // 1: bf16 storage mode: the large gather GEMMs by k_conv_gemm_f16 (weights global -> VGPR, 256 x 128 tiles); 2: regardless of the
  // launch size (tests).  The fragment-order twins of the weight images are written only while the option is on
  int conv_f16 = 1;
  // 1: bf16 storage mode, ndomain 16: forward of critic layer 2 by k_d2_fwd_slab16 (measured: no faster than the streaming GEMM, default off)
  int d2_fwd_slab = 0;
  // 1: the slab kernel of layer 2's input gradient reads the packed gate instead of layer 1's output
  int d2_gate_bits = 1;
  // 1: bf16 storage mode, ndomain 16: input gradient of critic layer 2 by k_d2_dgrad_slab16
  int d2_slab = 1;
  // tests: force the row-slice count of the critic Dense weight gradient (0 = by batch size)
  int dense_slices = 0;
  // test hook "keep_gates": the critic step's second sweep overwrites the x_hat third of h_l in place; with the option on, that third
  // is copied to RdTestHooks::gate_keep first, so that rdgan_debug_activation can return the activations (= LeakyReLU / dropout
  // pattern) of all 3B samples of the last critic step
  int keep_gates = 0;
  // 1: fp32 conv GEMMs of the producer/consumer kernel multiply on the bf16 matrix pipe from 3-way split operands (optional data point)
  int split3 = 0;
  // option "side_stream": weight-only kernels and bias-gradient column sums beside the caller's stream (see RdStreams)
  int side_on = 1;
  // option "gen_fwd_ahead" (see RdStreams): 1 on, 0 off, -1 by storage mode: on with fp32 storage (the metric: 11.03 -> 10.77 ms), off
  // in the bf16 mode, whose critic tail leaves no CUs idle (BASELINE configs[2] / [4] shard 0.3-0.6 % slower)
  int fwd_ahead = -1;
  // 1: dedicated streaming kernels for the generator's last conv (rdgan_edge.hip.h); 0: the tiled GEMM kernels; 2: also with fp32 storage
  int edge_kernels = 1;
  // global index of this rank's first sample: RandomWeightedAverage's alpha of sample k is uniform(key, sample_offset + k)
  int sample_offset = 0;
  // 1: split K of mid-size producer/consumer launches to fill whole rounds of workgroups; 0: off; >1: force (tests)
  int ws_ksplit = 1;
};

// the cached weight forms an option shapes
enum { RD_FORMS_GEN = 1, RD_FORMS_CRITIC = 2 };

// how rdgan_set_option normalises the caller's value; lo / hi bound every kind but RAW
enum RdOptKind { RD_OPT_BOOL, RD_OPT_TRISTATE, RD_OPT_CLAMP, RD_OPT_RANGE, RD_OPT_RAW };
#define RD_BOOL RD_OPT_BOOL, 0, 1                  // value ? 1 : 0
#define RD_TRISTATE RD_OPT_TRISTATE, -1, 1         // < 0 -> -1, else 0 / 1
#define RD_CLAMP(lo, hi) RD_OPT_CLAMP, lo, hi      // clamped into [lo, hi]
#define RD_RANGE(lo, hi) RD_OPT_RANGE, lo, hi      // refused outside [lo, hi], with the row's message
#define RD_RAW RD_OPT_RAW, 0, 0                    // stored as given

struct RdOptionRow {
  const char* name;
  const char* alias;          // legacy name, still accepted (or nullptr)
  int RdOptions::*field;
  RdOptKind kind; int lo, hi;
  unsigned forms;             // RD_FORMS_* the option shapes: part of that network's form key
  int def;                    // the default: RdOptions' initialiser (checked below)
  const char* refusal;        // RD_RANGE: the message of a refused value
};

static constexpr RdOptionRow RD_OPTIONS[] = {
  // name                 alias        field                         normalisation          forms shaped                     default
  {"collapse",            nullptr,     &RdOptions::collapse,         RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"wave_specialized",    nullptr,     &RdOptions::wave_spec,        RD_CLAMP(0, 2),        0,                               1, nullptr},
  {"bf16",                "mfma_bf16", &RdOptions::a16,              RD_BOOL,               RD_FORMS_GEN | RD_FORMS_CRITIC,  0, nullptr},
  {"g9_direct",           nullptr,     &RdOptions::g9_direct,        RD_BOOL,               0,                               1, nullptr},
  {"fast_fwd",            nullptr,     &RdOptions::fast_fwd,         RD_TRISTATE,           RD_FORMS_GEN,                   -1, nullptr},
  {"fast_bwd",            nullptr,     &RdOptions::fast_bwd,         RD_TRISTATE,           0,                              -1, nullptr},
  {"tapgather",           nullptr,     &RdOptions::tapgather,        RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"resident",            nullptr,     &RdOptions::resident,         RD_BOOL,               0,                               1, nullptr},
  {"upconv_slab",         nullptr,     &RdOptions::upconv_slab,      RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"upconv_slab_t",       nullptr,     &RdOptions::upconv_slab_t,    RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"upconv2_slab",        nullptr,     &RdOptions::upconv2_slab,     RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"g9_fused",            nullptr,     &RdOptions::g9_fused,         RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"d1_fwd_sample",       nullptr,     &RdOptions::d1_fwd_sample,    RD_BOOL,               0,                               1, nullptr},
  {"g9_bwd_mfma",         nullptr,     &RdOptions::g9_bwd_mfma,      RD_BOOL,               0,                               1, nullptr},
  {"dense16",             nullptr,     &RdOptions::dense16,          RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"dense_skinny",        nullptr,     &RdOptions::dense_skinny,     RD_BOOL,               RD_FORMS_GEN,                    1, nullptr},
  {"wgrad_boxes",         nullptr,     &RdOptions::wgrad_boxes,      RD_BOOL,               0,                               1, nullptr},
  {"border_boxes",        nullptr,     &RdOptions::border_boxes,     RD_CLAMP(0, 2),        0,                               1, nullptr},
  {"d3_wgrad_slab",       nullptr,     &RdOptions::d3_wgrad_slab,    RD_BOOL,               0,                               1, nullptr},
  {"d2_wgrad_slab",       nullptr,     &RdOptions::d2_wgrad_slab,    RD_BOOL,               0,                               1, nullptr},
  {"upwgrad_slab",        nullptr,     &RdOptions::upwgrad_slab,     RD_BOOL,               0,                               1, nullptr},
  {"d1_dgrad_fused",      nullptr,     &RdOptions::d1_dgrad_fused,   RD_BOOL,               0,                               1, nullptr},
  {"combine_dx_fused",    nullptr,     &RdOptions::combine_dx_fused, RD_BOOL,               0,                               1, nullptr},
  {"d1_wgrad16",          nullptr,     &RdOptions::d1_wgrad16,       RD_BOOL,               0,                               1, nullptr},
  {"wgrad_wide",          nullptr,     &RdOptions::wgrad_wide,       RD_BOOL,               0,                               0, nullptr},
  {"conv_f16",            nullptr,     &RdOptions::conv_f16,         RD_RANGE(0, 2),        RD_FORMS_GEN | RD_FORMS_CRITIC,  1,
   "conv_f16: 0, 1 or 2 (2: regardless of the launch size)"},
  {"d2_fwd_slab",         nullptr,     &RdOptions::d2_fwd_slab,      RD_BOOL,               RD_FORMS_CRITIC,                 0, nullptr},
  {"d2_gate_bits",        nullptr,     &RdOptions::d2_gate_bits,     RD_BOOL,               0,                               1, nullptr},
  {"d2_slab",             nullptr,     &RdOptions::d2_slab,          RD_BOOL,               RD_FORMS_CRITIC,                 1, nullptr},
  {"dense_wgrad_slices",  nullptr,     &RdOptions::dense_slices,     RD_RAW,                0,                               0, nullptr},
  {"keep_gates",          nullptr,     &RdOptions::keep_gates,       RD_BOOL,               0,                               0, nullptr},
  {"split3",              nullptr,     &RdOptions::split3,           RD_BOOL,               0,                               0, nullptr},
  {"side_stream",         nullptr,     &RdOptions::side_on,          RD_BOOL,               0,                               1, nullptr},
  {"gen_fwd_ahead",       nullptr,     &RdOptions::fwd_ahead,        RD_TRISTATE,           0,                              -1, nullptr},
  {"edge_kernels",        nullptr,     &RdOptions::edge_kernels,     RD_CLAMP(0, 2),        0,                               1, nullptr},
  {"sample_offset",       nullptr,     &RdOptions::sample_offset,    RD_RANGE(0, INT_MAX),  0,                               0,
   "set_option: sample_offset < 0"},
  {"ws_ksplit",           nullptr,     &RdOptions::ws_ksplit,        RD_CLAMP(0, 8),        0,                               1, nullptr},
};
constexpr int RD_NUM_OPTIONS = (int)(sizeof(RD_OPTIONS) / sizeof(RD_OPTIONS[0]));

// every row's default is its field's initialiser; a row that shapes forms has a bounded value, and a network's key fits an int
constexpr bool rd_options_table_ok() {
  const RdOptions o{};
  for (unsigned forms = RD_FORMS_GEN; forms <= RD_FORMS_CRITIC; forms <<= 1) {
    long span = 1;
    for (int i = 0; i < RD_NUM_OPTIONS; ++i) {
      const RdOptionRow& r = RD_OPTIONS[i];
      if (o.*r.field != r.def) return false;
      if (!(r.forms & forms)) continue;
      if (r.kind == RD_OPT_RAW) return false;
      span *= (long)r.hi - r.lo + 1;
      if (span > INT_MAX) return false;
    }
  }
  return true;
}
static_assert(rd_options_table_ok(), "RD_OPTIONS: a default differs from RdOptions' initialiser, or a form-shaping row is unbounded");

static inline const RdOptionRow* rd_option_find(const char* name) {
  for (const RdOptionRow& r : RD_OPTIONS)
    if (!strcmp(name, r.name) || (r.alias && !strcmp(name, r.alias))) return &r;
  return nullptr;
}

// the value the option takes for a caller's `value`; false: refused (RD_RANGE), *out untouched
static inline bool rd_option_normalise(const RdOptionRow& r, int value, int* out) {
  switch (r.kind) {
    case RD_OPT_BOOL: *out = value ? 1 : 0; return true;
    case RD_OPT_TRISTATE: *out = value < 0 ? -1 : (value ? 1 : 0); return true;
    case RD_OPT_CLAMP: *out = value < r.lo ? r.lo : (value > r.hi ? r.hi : value); return true;
    case RD_OPT_RANGE: if (value < r.lo || value > r.hi) return false; *out = value; return true;
    case RD_OPT_RAW: break;
  }
  *out = value;
  return true;
}

// the option state the weight forms of one network (RD_FORMS_GEN / RD_FORMS_CRITIC) depend on, as one non-negative number: the
// values of the rows flagged for it, mixed-radix.  Two states that build different forms differ in the key (it may be finer: the
// raw values, not the predicates the builders derive from them)
static inline int rd_form_key(const RdOptions* o, unsigned forms) {
  int key = 0;
  for (const RdOptionRow& r : RD_OPTIONS)
    if (r.forms & forms) key = key * (r.hi - r.lo + 1) + (o->*r.field - r.lo);
  return key;
}
