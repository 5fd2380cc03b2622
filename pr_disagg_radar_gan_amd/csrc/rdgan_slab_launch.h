// Host launchers of the hand-written slab kernels of the bf16 storage mode, one per kernel: grid, dynamic LDS, group count,
// partial-slab size, fold / reduce launch, profiling scopes and launch record.  The training step and the op-level entry points
// (rdgan_op_*) both launch through these, so a parity test runs the launch the step performs.  Included by rdgan_api.hip behind
// ProfScope / LaunchScope / RD_KNAME; the handle may be nullptr (op-level entries), as in the launch_conv family.
#pragma once

// what differs between the call sites of one launcher: the launch record's plan index and FLOPs, and the profiling tag
struct SlabRec { int plan; double flops; int tag; };
static const SlabRec kOpRec = {-1, 0.0, -1};          // op-level entries: no plan, no tag

// profiling scope + launch record + kernel name + FLOP count of one slab launch
struct SlabScope {
  ProfScope ps; LaunchScope ls;
  SlabScope(rdgan_handle* h, const SlabRec& r, int kind, int batch, hipStream_t st, const char* name)
      : ps(h, r.tag, st), ls(h, r.plan, kind, batch, r.flops, st) {
    RD_KNAME(h, "%s", name);
    if (h) h->flops_acc += r.flops;
  }
};

// ---- weight images (fp32 weights -> the fragment-order bf16 image its slab kernel streams)
static void launch_upconv_wimg(const float* wc, void* img, hipStream_t st) {
  hipLaunchKernelGGL(k_upconv_wimg, dim3(256), dim3(256), 0, st, wc, (unsigned short*)img);
}
static void launch_upconv_wimg_t(const float* wc, void* img, hipStream_t st) {
  hipLaunchKernelGGL(k_upconv_wimg_t, dim3(256), dim3(256), 0, st, wc, (unsigned short*)img);
}
static void launch_upconv2_wimg(const float* wc, void* img, hipStream_t st) {
  hipLaunchKernelGGL(k_upconv2_wimg, dim3(RD_UP2_KSTEPS), dim3(256), 0, st, wc, (unsigned short*)img);
}
static void launch_d2s_wimg(const float* w2, void* img, hipStream_t st) {
  hipLaunchKernelGGL(k_d2s_wimg, dim3((RD_D2S_KSTEPS * 2 * 64 + 255) / 256), dim3(256), 0, st, w2, (unsigned short*)img);
}
static void launch_d2f_wimg(const float* w2, void* img, hipStream_t st) {
  hipLaunchKernelGGL(k_d2f_wimg, dim3(RD_D2F_KSTEPS), dim3(256), 0, st, w2, (unsigned short*)img);
}

// ---- generator block 3 forward, ndomain 16 (k_upconv_slab16<NAMETAG>).  w9img != nullptr: + the last conv's tap products (Q12)
// from the rows while they are in registers, with (store_h3) or without the block's own output; NAMETAG = 1 only
template <int NAMETAG>
static int launch_upconv_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* wimg, const float* bias, void* out, float* rinv,
                              int B, float* dbg, const void* w9img, float* Q12, bool store_h3, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_CONV, B, st, w9img ? "k_upconv_slab16<bf16, +conv 64->1>" : "k_upconv_slab16<bf16>");
  const dim3 ug((unsigned)std::min(6 * B, 512));
  if (!w9img) {
    RD_TRY(ensure_lds(h, (const void*)k_upconv_slab16<NAMETAG>, RD_UPC_LDS));
    hipLaunchKernelGGL(k_upconv_slab16<NAMETAG>, ug, dim3(256), RD_UPC_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)wimg, bias,
                       (rd_bf16_t*)out, rinv, B, dbg);
  } else if constexpr (NAMETAG == 1) {
    auto kern = store_h3 ? k_upconv_slab16<1, true, true> : k_upconv_slab16<1, true, false>;
    RD_TRY(ensure_lds(h, (const void*)kern, RD_UPC_LDS_G9));
    hipLaunchKernelGGL(kern, ug, dim3(256), RD_UPC_LDS_G9, st, (const rd_bf16_t*)x, (const rd_bf16_t*)wimg, bias, (rd_bf16_t*)out, rinv, B,
                       dbg, (const unsigned short*)w9img, Q12);
  } else
    return bad_arg(h, "upconv slab: the fused last conv runs under NAMETAG 1 only");
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// the same on (h, w) tiles of source planes of Hs x Ws positions, multiples of 8 (k_upconv_slab_t16)
static int launch_upconv_slab_t(rdgan_handle* h, const SlabRec& r, const void* x, const void* wimg, const float* bias, void* out, float* rinv,
                                int B, int Hs, int Ws, float* dbg, const void* w9img, float* Q12, bool store_h3, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_CONV, B, st, w9img ? "k_upconv_slab_t16<bf16, +conv 64->1>" : "k_upconv_slab_t16<bf16>");
  const long items = (long)B * 6 * (Hs / 8) * (Ws / 8);
  auto kern = !w9img ? k_upconv_slab_t16<false, true> : store_h3 ? k_upconv_slab_t16<true, true> : k_upconv_slab_t16<true, false>;
  const size_t lds = w9img ? RD_UPT_LDS_G9 : RD_UPT_LDS;
  RD_TRY(ensure_lds(h, (const void*)kern, lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)std::min<long>(items, 512)), dim3(256), lds, st, (const rd_bf16_t*)x, (const rd_bf16_t*)wimg, bias,
                     (rd_bf16_t*)out, rinv, B, Hs, Ws, dbg, (const unsigned short*)w9img, Q12);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// generator block 2 forward, ndomain 16 (k_upconv2_slab16)
static int launch_upconv2_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* wimg, const float* bias, void* out, float* rinv,
                               int B, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_CONV, B, st, "k_upconv2_slab16<bf16>");
  RD_TRY(ensure_lds(h, (const void*)k_upconv2_slab16, RD_UP2_LDS));
  hipLaunchKernelGGL(k_upconv2_slab16, dim3((unsigned)std::min(B, 256 * RD_UP2_WGS)), dim3(256), RD_UP2_LDS, st, (const rd_bf16_t*)x,
                     (const rd_bf16_t*)wimg, bias, (rd_bf16_t*)out, rinv, B);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ---- critic layer 2 forward, ndomain 16 (k_d2_fwd_slab16)
static int launch_d2_fwd_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* wimg, const float* bias, void* out, int B,
                              int use_drop, uint32_t key, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_CONV, B, st, "k_d2_fwd_slab16<bf16>");
  RD_TRY(ensure_lds(h, (const void*)k_d2_fwd_slab16, RD_D2F_LDS));
  hipLaunchKernelGGL(k_d2_fwd_slab16, dim3((unsigned)std::min(B, 512)), dim3(256), RD_D2F_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)wimg,
                     bias, (rd_bf16_t*)out, B, use_drop, key, 0u);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ---- critic layer 2 input gradient: two samples per workgroup pass (k_d2_dgrad_slab16, ndomain 16); gbits: layer 1's packed gate or nullptr
static int launch_d2_dgrad_slab(rdgan_handle* h, const SlabRec& r, const void* gy, const void* wimg, const void* aux, void* gx, int B,
                                int use_drop, const unsigned char* gbits, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_CONV, B, st, "k_d2_dgrad_slab16<bf16>");
  RD_TRY(ensure_lds(h, (const void*)k_d2_dgrad_slab16, RD_D2S_LDS));
  hipLaunchKernelGGL(k_d2_dgrad_slab16, dim3((unsigned)std::min((B + 1) / 2, 512)), dim3(256), RD_D2S_LDS, st, (const rd_bf16_t*)gy,
                     (const rd_bf16_t*)wimg, (const rd_bf16_t*)aux, (rd_bf16_t*)gx, B, use_drop, gbits);
  RD_CHECK(h, hipGetLastError());
  return 0;
}
// the same on tiles of 4 x 4 output-gradient positions (k_d2_dgrad_slab_t16): OH, OW multiples of 4
static int launch_d2_dgrad_slab_t(rdgan_handle* h, const SlabRec& r, const void* gy, const void* wimg, const void* aux, void* gx, int B,
                                  int OH, int OW, int use_drop, const unsigned char* gbits, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_CONV, B, st, "k_d2_dgrad_slab_t16<bf16>");
  const long items = (long)((B + 1) / 2) * (OH / 4) * (OW / 4);
  RD_TRY(ensure_lds(h, (const void*)k_d2_dgrad_slab_t16, RD_D2T_LDS));
  hipLaunchKernelGGL(k_d2_dgrad_slab_t16, dim3((unsigned)std::min<long>(items, 512)), dim3(256), RD_D2T_LDS, st, (const rd_bf16_t*)gy,
                     (const rd_bf16_t*)wimg, (const rd_bf16_t*)aux, (rd_bf16_t*)gx, B, OH, OW, use_drop, gbits);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ---- critic layer 2 weight gradient: G groups of workgroups share the batch, partial [G][27][64][128], then the fold.
// items = samples (ndomain 16) or samples x tiles (tiled kernel)
constexpr int RD_D2W_GMAX = 64;
static int d2w_groups(long items) { return items >= 64 ? RD_D2W_GMAX : 8; }
static size_t d2w_partial_floats(int G) { return (size_t)G * 27 * RD_D2W_TILE; }
// geo == nullptr: k_d2_wgrad_slab16 (ndomain 16); otherwise k_d2_wgrad_slab_t16 on geo's tiles of 4 x 4 output positions
static int launch_d2_wgrad_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* dy, float* partial, size_t partial_cap,
                                float* dW, int B, const RdD2wGeom* geo, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_WGRAD, B, st, geo ? "k_d2_wgrad_slab_t16<bf16>" : "k_d2_wgrad_slab16<bf16>");
  const int G = d2w_groups(geo ? (long)B * geo->TH * geo->TW : (long)B);
  if (d2w_partial_floats(G) > partial_cap) return bad_arg(h, "d2 wgrad: partial workspace too small");
  if (geo) {
    RD_TRY(ensure_lds(h, (const void*)k_d2_wgrad_slab_t16, RD_D2WT_LDS));
    hipLaunchKernelGGL(k_d2_wgrad_slab_t16, dim3(4 * G), dim3(512), RD_D2WT_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)dy, partial, B, G,
                       *geo);
  } else {
    RD_TRY(ensure_lds(h, (const void*)k_d2_wgrad_slab16, RD_D2W_LDS));
    hipLaunchKernelGGL(k_d2_wgrad_slab16, dim3(4 * G), dim3(512), RD_D2W_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)dy, partial, B, G);
  }
  hipLaunchKernelGGL(k_d2_wgrad_fold, dim3((27 * RD_D2W_TILE / 4 + 255) / 256), dim3(256), 0, st, partial, G, dW);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ---- critic layer 3 weight gradient, ndomain 16 (k_d3_wgrad_slab16): partial [G][27][128][256]
constexpr int RD_D3W_GMAX = 16;
static int d3w_groups(int B) { return B >= 256 ? RD_D3W_GMAX : 8; }
static size_t d3w_partial_floats(int G) { return (size_t)G * 27 * RD_D3W_TILE; }
static int launch_d3_wgrad_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* dy, float* partial, size_t partial_cap,
                                float* dW, int B, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_WGRAD, B, st, "k_d3_wgrad_slab16<bf16>");
  const int G = d3w_groups(B);
  if (d3w_partial_floats(G) > partial_cap) return bad_arg(h, "d3 wgrad: partial workspace too small");
  RD_TRY(ensure_lds(h, (const void*)k_d3_wgrad_slab16, RD_D3W_LDS));
  hipLaunchKernelGGL(k_d3_wgrad_slab16, dim3(16 * G), dim3(512), RD_D3W_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)dy, partial, B, G);
  hipLaunchKernelGGL(k_d3_wgrad_fold, dim3((27 * RD_D3W_TILE / 4 + 255) / 256), dim3(256), 0, st, partial, G, dW);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ---- collapsed weight gradient of generator block 3, ndomain 16 (k_upconv_wgrad_slab16): partial [G][64][128][64].  bias_part (optional,
// [8 G][64]): the bias gradient's partial rows, folded into db
constexpr int RD_UWG_GMAX = 32;
static int upwgrad_groups(int B) { return 6 * B >= 64 ? RD_UWG_GMAX : 8; }
static size_t upwgrad_partial_floats(int G) { return (size_t)G * 64 * RD_UWG_TILE; }
static int launch_upconv_wgrad_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* dy, float* partial, size_t partial_cap,
                                    float* dWc, float* bias_part, float* db, int B, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_WGRAD, B, st, "k_upconv_wgrad_slab16<bf16>");
  const int G = upwgrad_groups(B);
  if (upwgrad_partial_floats(G) > partial_cap) return bad_arg(h, "upconv wgrad: partial workspace too small");
  RD_TRY(ensure_lds(h, (const void*)k_upconv_wgrad_slab16, RD_UWG_LDS));
  hipLaunchKernelGGL(k_upconv_wgrad_slab16, dim3(8 * G), dim3(512), RD_UWG_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)dy, partial, B, G,
                     bias_part);
  hipLaunchKernelGGL(k_upconv_wgrad_fold, dim3(64 * RD_UWG_TILE / 4 / 256), dim3(256), 0, st, partial, G, dWc);
  if (bias_part)      // (a serial fold of the 256 partial rows took 61 us)
    hipLaunchKernelGGL(k_reduce_partials, dim3(64 / 16), dim3(rd_reduce_threads(8 * G)), 0, st, bias_part, 8 * G, 64, db);
  RD_CHECK(h, hipGetLastError());
  return 0;
}
// the same on block 2's geometry (k_upconv2_wgrad_slab16): partial [G][64][256][128], bias partials [8 G][128]
constexpr int RD_UW2_GROUPS = 8;
static size_t upwgrad2_partial_floats() { return (size_t)RD_UW2_GROUPS * 64 * RD_UW2_TILE; }
static int launch_upconv2_wgrad_slab(rdgan_handle* h, const SlabRec& r, const void* x, const void* dy, float* partial, size_t partial_cap,
                                     float* dWc, float* bias_part, float* db, int B, hipStream_t st) {
  SlabScope sc(h, r, RD_KIND_WGRAD, B, st, "k_upconv2_wgrad_slab16<bf16>");
  constexpr int G = RD_UW2_GROUPS;
  if (upwgrad2_partial_floats() > partial_cap) return bad_arg(h, "upconv wgrad: partial workspace too small");
  RD_TRY(ensure_lds(h, (const void*)k_upconv2_wgrad_slab16, RD_UW2_LDS));
  hipLaunchKernelGGL(k_upconv2_wgrad_slab16, dim3(32 * G), dim3(512), RD_UW2_LDS, st, (const rd_bf16_t*)x, (const rd_bf16_t*)dy, partial, B, G,
                     bias_part);
  hipLaunchKernelGGL(k_upconv2_wgrad_fold, dim3(64 * RD_UW2_TILE / 4 / 256), dim3(256), 0, st, partial, G, dWc);
  if (bias_part) hipLaunchKernelGGL(k_reduce_partials, dim3(128 / 16), dim3(rd_reduce_threads(8 * G)), 0, st, bias_part, 8 * G, 128, db);
  RD_CHECK(h, hipGetLastError());
  return 0;
}

// ---- weight gradient of the last generator conv (64 -> 1) [27][64]: the matrix-pipe kernel (k_g9_wgrad_mfma: persistent, three
// workgroups per CU, needs g9w_mfma_ok) or the scalar kernel (k_g9_wgrad_pairs: one (sample, plane pair) unit per workgroup up to
// 3072), then the fold of the workgroups' partial rows.  Only the matrix-pipe launch is recorded.
static int g9w_groups(bool mfma, int B, int nd) {
  return mfma ? (int)std::min<long>(((long)B * RDGAN_NHOURS * nd * nd + 127) / 128, 768) : std::min(B * (RDGAN_NHOURS / 2), 3072);
}
static size_t g9w_partial_floats(int nwg) { return (size_t)nwg * 1728; }
static size_t g9_pairs_lds(int nd) { return std::max<size_t>(4 * (size_t)(nd + 2) * (nd + 2) * sizeof(float), 4 * 27 * 16 * sizeof(f32x4)); }
static int launch_g9_wgrad(rdgan_handle* h, const SlabRec& r, bool mfma, bool a16, const float* dl, const void* h3, float* partial,
                           size_t partial_cap, float* dW, int B, int nd, hipStream_t st) {
  ProfScope ps(h, r.tag, st);
  const int D = RDGAN_NHOURS, nwg = g9w_groups(mfma, B, nd);
  if (g9w_partial_floats(nwg) > partial_cap) return bad_arg(h, "g9 wgrad: partial workspace too small");
  if (mfma) {
    const long npix = (long)B * D * nd * nd;
    const size_t lds = g9w_mfma_lds(a16);
    RD_TRY(ensure_lds(h, a16 ? (const void*)k_g9_wgrad_mfma<rd_bf16_t> : (const void*)k_g9_wgrad_mfma<float>, lds));
    LaunchScope ls(h, r.plan, RD_KIND_WGRAD, B, r.flops, st);
    RD_KNAME(h, "k_g9_wgrad_mfma<%s>", a16 ? "bf16" : "f32");
    if (h) h->flops_acc += r.flops;
    if (a16) hipLaunchKernelGGL(k_g9_wgrad_mfma<rd_bf16_t>, dim3(nwg), dim3(256), lds, st, dl, (const rd_bf16_t*)h3, partial, npix, D, nd, nd,
                                ilog2(nd));
    else hipLaunchKernelGGL(k_g9_wgrad_mfma<float>, dim3(nwg), dim3(256), lds, st, dl, (const float*)h3, partial, npix, D, nd, nd, ilog2(nd));
  } else {
    const size_t lds = g9_pairs_lds(nd);
    if (lds > 96 * 1024) return bad_arg(h, "g9 wgrad: the hour planes do not fit in LDS");
    RD_TRY(ensure_lds(h, a16 ? (const void*)k_g9_wgrad_pairs<rd_bf16_t> : (const void*)k_g9_wgrad_pairs<float>, 96 * 1024));
    const int nunits = B * (D / 2);
    if (a16) hipLaunchKernelGGL(k_g9_wgrad_pairs<rd_bf16_t>, dim3(nwg), dim3(256), lds, st, dl, (const rd_bf16_t*)h3, partial, D, nd, nd, nunits);
    else hipLaunchKernelGGL(k_g9_wgrad_pairs<float>, dim3(nwg), dim3(256), lds, st, dl, (const float*)h3, partial, D, nd, nd, nunits);
  }
  hipLaunchKernelGGL(k_reduce_partials, dim3((1728 + 15) / 16), dim3(rd_reduce_threads(nwg)), 0, st, partial, nwg, 1728, dW);
  RD_CHECK(h, hipGetLastError());
  return 0;
}
