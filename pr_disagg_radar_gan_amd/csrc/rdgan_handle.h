// struct rdgan_handle, grouped by concern, and what every launcher needs of it: the error macros, side-stream fork / join, the
// per-handle dynamic-LDS record and the profiling scopes.  Host code, included by rdgan_api.hip behind the kernel headers (it uses
// RdGeom / RdPlan / RdRow of rdgan_hostplan.h / rdgan_plan.h and the HIP runtime types).  The handle inherits plain base structs,
// so a field is spelled h->collapse, h->h3, h->gcache_ver whatever group it lives in.
#pragma once
#include "rdgan_options.h"      // RdOptions: every integer rdgan_set_option writes

static_assert(RDGAN_LOSS_SLOTS == 8, "k_critic_losses / k_gen_loss write slots 0..7");
// k_g9_wgrad_mfma: W a power of two in [8, 128]; dynamic LDS = tile + staged dlogits rows + row descriptors (>= the 32 KB fold)
static bool g9w_mfma_ok(int nd, long npix) { return nd >= 8 && nd <= 128 && (nd & (nd - 1)) == 0 && npix < 0x7FFFFFFFL; }
static size_t g9w_mfma_lds(bool bf16) { return std::max<size_t>((size_t)128 * (bf16 ? 128 : 256) + (1440 + 144) * sizeof(float), 32768); }

#define RD_GP_WEIGHT 10.0f   // the literal at T:392

// one GEMM launch under rdgan_profile_launches: which plan, through which kernel, how many samples and algorithmic FLOPs
struct RdLaunchRec { int plan, kind, batch; double flops; char kernel[48]; hipEvent_t e0, e1; };

// the plan tables and the workspace: one allocation, carved by rdgan_create into every pointer below
struct RdWorkspace {
  // plans: host copies, their device copies, and the device row table the plans point into
  std::vector<RdPlan> plans;
  RdPlan* d_plans = nullptr;
  RdRow* d_tab = nullptr;
  // the workspace allocation
  char* ws = nullptr;
  size_t ws_bytes = 0;
  // generator activations, 1/l2 of PixelNorm, the last conv's tap sums and output, and the backward's gradients
  float *xcat, *h0, *h1, *r1, *h2, *r2, *h3, *r3, *P9, *fake, *dl, *gh3, *gup3, *dy2, *gup2, *dy1, *gup1, *ga0;
  // critic input, per layer activations dh / output gradients du, values, layer-1 column matrix, dD/d(sample), penalty terms
  float *cin, *dh[5], *du[5], *v, *P1, *g0, *gpv;
  // k_upconv_wgrad_slab16's bias-gradient partials [32 groups][8 phases][64]
  float* ubias_part = nullptr;
  // partial slabs: streaming weight gradients, column sums, split-K; their capacities in floats
  float *wpartial, *cpartial, *kpartial;
  size_t wpartial_cap = 0, cpartial_cap = 0, kpartial_cap = 0;
  // transposed critic kernels (input-gradient GEMMs), layer 1 transposed, direct generator forms, the 64 -> 1 kernel [64][32],
  // layer 1 zero-padded to CP channels and its gradient
  float *DWT[5], *W1T, *GWT[4], *W9T, *W1P, *dW1P;
  // shared-centre form: per block the hour differences E of its input and the 48 weight forms U (written by the forward,
  // reused by the backward); T / plane sums gS, the gradient wrt E, weight-form gradients and transposes (scratch)
  float *fE[4], *fU[4], *fgS, *fdE, *fdU, *fUT;
  // "bf16" storage mode: activations and activation gradients live in the workspace as bf16 (the same float* fields then
  // point at bf16 data; act_off() does their pointer arithmetic); bf16 weight images of every bf16-MFMA GEMM, rebuilt from
  // the fp32 master weights inside each call: shared-centre forms [48][N][K] and their tap-reordered input-gradient
  // stack, critic layers 2-4 forward [27][Cout][Cin] / input gradient [27][Cin][Cout], generator block 1 collapsed forms
  // [64][Cout][Cin] and (re-ordered by tap) [64][Cin][Cout], the first critic kernel [ldp1][64]
  void *bU[4], *bUT;
  void *bWF[5], *bWB[5];
  void *bG1F[4], *bG1B, *bW1B;
  // the same images in fragment order (rdgan_gemm_f16.hip.h: rd_wfrag_index), written beside them
  void *fWF[5], *fWB[5], *fG1F[4], *fG1B;
  // weight image of the slab kernel of generator block 3 (rdgan_upconv16.hip.h): 1 MB, MFMA-fragment order
  void* bW3I;
  // weight image of the TILED slab kernel of generator block 3 (rdgan_upconv16t.hip.h): 1 MB, [phase][half][tap][j]
  void* bW3T = nullptr;
  // weight image of the slab kernel of generator block 2 (rdgan_upconv16b.hip.h): 4 MB
  void* bW2I = nullptr;
  // A-fragment image of the 64 -> 1 kernel for the block-3 slab kernel's epilogue ("g9_fused", k_g9_wimg): 4 KB
  void* bW9I;
  // weight image of the slab kernel of critic layer 2's input gradient (rdgan_d2slab16.hip.h): 432 KB
  void* bW2S;
  // weight image of the slab kernel of critic layer 2's forward (rdgan_d2fwd16.hip.h): 448 KB
  void* bW2F = nullptr;
  // layer 1's gate in 2 bits per element (written by k_d1_gemm_fwd, read by k_d2_dgrad_slab16): 16 B per row
  unsigned char* g1bits = nullptr;
  // the Dense layer on the bf16 matrix pipe: input rows [MB][KP0] bf16
  void* xcat16 = nullptr;
  // ... and its kernel [n_nodes][KP0] bf16
  void* bW0 = nullptr;
  // collapsed generator weights, their dgrad form, collapsed wgrad scratch
  float *GWC[4], *GWD[4], *dWc;
  // 64 partial sums of the last conv's bias gradient
  float* g9b_tmp;
  // [max_batch][64] partial sums of squares of the penalty's per-sample gradient norm
  float* gp_part;
  // [16][F] row-slice partial sums of the critic Dense weight gradient
  float* dw6_part;
  // the non-finite flag of the generator's softmax (rdgan_check_numerics)
  int* d_flag;
  // the early generator forward's own split-K slab and non-finite flag (see RdStreams)
  float* kpartial_ahead = nullptr;
  int* flag_ahead = nullptr;
};

// Weight-form cache (rdgan_set_weight_versions): the forward forms of the generator (W9T, collapsed / shared-centre forms, their
// bf16 images) and the critic's forms (transposes, padded / bf16 images) are functions of the weights alone.  The caller may
// assert a content version for each slab; a call whose (pointer, version, form options) equal those the forms in the
// workspace were built from skips the weight-only kernels.  Version 0 = unknown: rebuild (the default).
struct RdFormCache {
  // the versions the caller vouches for (0: none)
  uint64_t gver_in = 0, cver_in = 0;
  // what the generator's forms in the workspace were built from: slab, version, rd_form_key(h, RD_FORMS_GEN)
  const float* gcache_ptr = nullptr; uint64_t gcache_ver = 0; int gcache_cfg = -1;
  // the same for the critic's (RD_FORMS_CRITIC)
  const float* ccache_ptr = nullptr; uint64_t ccache_ver = 0; int ccache_cfg = -1;
  // how many times the generator / critic forms were (re)built (tests)
  long form_builds[2] = {0, 0};
};

// Side stream (option "side_stream", default on): weight-only kernels (generator weight forms, critic weight transposes /
// bf16 images) and the bias-gradient column sums run beside the caller's stream, ordered by events: ~50 launches of 5-30 us
// per iteration that would otherwise sit between the GEMMs.  Same kernels, same arithmetic: results are bit-identical.
//
// Generator forward ahead (option "gen_fwd_ahead", default on with fp32 storage; rdgan_critic_grad_ahead): the last critic
// step of an iteration issues the NEXT generator step's forward on a stream of its own, forked right after the critic input
// is built (from there
// on the critic step reads neither h->fake nor any generator activation), beside the critic step's tail and the caller's
// Adam.  The generator step then skips its forward and waits for ev_ahead_done in front of its critic forward.  Same kernels,
// same plans and splits: results are bit-identical to the option off.  What the early forward writes, against what the rest
// of the critic step touches (compute stream st, side stream for the column sums):
//   buffer                                   early forward (stream `ahead`)   critic step tail (st / side)
//   xcat, xcat16, h0..h3, r1..r3, fE, fgS, P9, fake   written                  not touched (fake read only by the build, before the fork)
//   generator weight forms (uncached only)    written                          not touched
//   kpartial (split-K partials)               kpartial_ahead (own copy)        kpartial
//   non-finite flag                           flag_ahead (own copy)            d_flag (read by k_critic_losses)
//   cin, dh, du, v, P1, g0, gpv, gp_part, wpartial, cpartial, dW1P, dw6_part, g1bits, critic forms: tail only
// Every other entry that uses the workspace first waits for a forward still pending (ahead_drain).
struct RdStreams {
  // the side stream (nullptr: it could not be created, the option stays off)
  hipStream_t side = nullptr;
  // fork / join of the side stream, the critic's forms complete, generator block l's forms complete
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_cw = nullptr, ev_g[4] = {nullptr, nullptr, nullptr, nullptr};
  // the early forward's stream and its fork / completion events
  hipStream_t ahead = nullptr;
  hipEvent_t ev_ahead_fork = nullptr, ev_ahead_done = nullptr;
  // a forward has been issued and not yet consumed / waited for
  bool ahead_pending = false;
  // ... and what it was issued with: the generator step consumes it only for the same slab, inputs, batch and version
  const float *ahead_gp = nullptr, *ahead_z = nullptr, *ahead_cond = nullptr;
  int ahead_B = 0;
  uint64_t ahead_gver = 0;
  // kernels whose dynamic-LDS limit has been raised on THIS handle's device (hipFuncSetAttribute is per device; keeping the
  // record per handle rather than per process makes two handles on two devices, or on two threads, independent)
  std::unordered_set<const void*> lds_attr_done;
};

// test hook "keep_gates" (RdOptions::keep_gates): the x_hat third of each critic layer's activations, copied before the second
// sweep overwrites it.  Allocated when the option is set, never inside a step.
struct RdTestHooks {
  void* gate_keep[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // samples held (0: the last call was not a critic step)
  int gate_keep_B = 0;
};

struct RdProfiling {
  // per-launch profiling (rdgan_profile_launches / rdgan_launch_table): HIP events around every GEMM launch
  int prof_launches = 0;
  std::vector<RdLaunchRec> launch_recs;
  size_t launch_used = 0;
  // tile name of the launch being issued (set by the launchers while prof_launches is on)
  char cur_kernel[48] = {0};
  // algorithmic FLOPs (2 * rows * taps * K * N of the forms actually run) of every GEMM launched so far
  double flops_acc = 0;
  // per-tag timing (rdgan_profile): the enabled tags and their event pairs
  unsigned prof_mask = 0;
  std::vector<hipEvent_t> ev_start[RDGAN_NUM_TAGS], ev_stop[RDGAN_NUM_TAGS];
  size_t ev_used[RDGAN_NUM_TAGS] = {0};
};

// RdGeom: geometry + parameter layout (rdgan_hostplan.h)
struct rdgan_handle : RdGeom, RdOptions, RdWorkspace, RdFormCache, RdStreams, RdTestHooks, RdProfiling {
  std::string err;      // rdgan_last_error
};

#define RD_CHECK(h, call)                                                        \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      char b_[512];                                                              \
      snprintf(b_, sizeof b_, "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      if (h) (h)->err = b_;                                                      \
      return (int)e_;                                                            \
    }                                                                            \
  } while (0)
#define RD_TRY(expr)            \
  do {                          \
    int r_ = (expr);            \
    if (r_ != 0) return r_;     \
  } while (0)

static int bad_arg(rdgan_handle* h, const char* msg) {
  if (h) h->err = msg;
  return -2;
}

// side stream ordered behind everything issued on `st` so far (or `st` itself with the option off)
static hipStream_t side_fork(rdgan_handle* h, hipStream_t st) {
  if (!h || !h->side_on || !h->side) return st;
  if (hipEventRecord(h->ev_fork, st) != hipSuccess || hipStreamWaitEvent(h->side, h->ev_fork, 0) != hipSuccess) return st;
  return h->side;
}
// `st` waits for everything issued on the side stream so far
static int side_join(rdgan_handle* h, hipStream_t st, hipEvent_t ev);

// raise a kernel's dynamic shared-memory limit once per handle (always, for the handle-less op-level entry points)
static int ensure_lds(rdgan_handle* h, const void* kern, size_t lds) {
  if (h && h->lds_attr_done.count(kern)) return 0;
  RD_CHECK(h, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (h) h->lds_attr_done.insert(kern);
  return 0;
}

static int side_join(rdgan_handle* h, hipStream_t st, hipEvent_t ev) {
  if (!h || !h->side_on || !h->side || st == h->side) return 0;
  RD_CHECK(h, hipEventRecord(ev, h->side));
  RD_CHECK(h, hipStreamWaitEvent(st, ev, 0));
  return 0;
}

struct ProfScope {
  rdgan_handle* h; int tag; hipStream_t st; bool on;
  ProfScope(rdgan_handle* h_, int tag_, hipStream_t st_) : h(h_), tag(tag_), st(st_), on(false) {
    if (h && tag >= 0 && (h->prof_mask >> tag & 1u) && h->ev_used[tag] < h->ev_start[tag].size()) {
      on = true;
      (void)hipEventRecord(h->ev_start[tag][h->ev_used[tag]], st);
    }
  }
  ~ProfScope() {
    if (on) { (void)hipEventRecord(h->ev_stop[tag][h->ev_used[tag]], st); h->ev_used[tag]++; }
  }
};

// plan index of a plan that lives in the handle's table (-1: a temporary plan of the op-level entry points)
static int plan_index(const rdgan_handle* h, const RdPlan& hp) {
  if (!h || h->plans.empty()) return -1;
  const RdPlan* b = h->plans.data();
  return (&hp >= b && &hp < b + h->plans.size()) ? (int)(&hp - b) : -1;
}
// kinds of a recorded launch
enum { RD_KIND_CONV = 0, RD_KIND_WGRAD = 1, RD_KIND_EDGE = 2 };
struct LaunchScope {
  rdgan_handle* h; hipStream_t st; RdLaunchRec* r;
  LaunchScope(rdgan_handle* h_, int plan, int kind, int batch, double flops, hipStream_t st_) : h(h_), st(st_), r(nullptr) {
    if (h && h->prof_launches && h->launch_used < h->launch_recs.size()) {
      r = &h->launch_recs[h->launch_used++];
      r->plan = plan; r->kind = kind; r->batch = batch; r->flops = flops; r->kernel[0] = 0;
      h->cur_kernel[0] = 0;
      (void)hipEventRecord(r->e0, st);
    }
  }
  ~LaunchScope() {
    if (r) { (void)hipEventRecord(r->e1, st); memcpy(r->kernel, h->cur_kernel, sizeof(r->kernel)); }
  }
};
#define RD_KNAME(h, ...) do { if ((h) && (h)->prof_launches) snprintf((h)->cur_kernel, sizeof((h)->cur_kernel), __VA_ARGS__); } while (0)
