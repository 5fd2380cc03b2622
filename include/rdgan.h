/* C ABI of librdgan_hip.so -- the MI355X-native (gfx950) cWGAN-GP hot path of RainDisaggGAN.
 *
 * The reference (sipposip/pr-disagg-radar-gan) has no native boundary: its hot path is a set of
 * Keras calls into TensorFlow 2.1.  Each entry point below names the reference call it replaces
 * (T = gan_train_cwgangp_pixelnorm.py, P = raindisagg_gan_pretrained.py).  The binding a
 * maintainer would add on the reference side is the ctypes stub in INTEGRATION.md /
 * pr_disagg_radar_gan_amd/_lib.py.
 *
 * Conventions: plain C, no torch types.  Every pointer is a DEVICE pointer owned by the caller
 * (fp32, 16-byte aligned); `stream` is a hipStream_t passed as void*; calls are asynchronous on
 * that stream and never allocate (the workspace is sized at rdgan_create).  Return value: 0 = ok,
 * >0 = hipError_t, -2 = bad argument.  One handle per device and per stream user; a handle is not
 * thread-safe.  Layouts are the reference's: activations NDHWC, Conv3D kernels
 * (kd,kh,kw,Cin,Cout), Dense kernels (in,out); parameter slabs are the Keras weights concatenated
 * in model.get_weights() order (kernel, bias per layer; see rdgan_*_param_layout).
 */
#ifndef RDGAN_H
#define RDGAN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rdgan_handle rdgan_handle;

#define RDGAN_LATENT_DIM 100   /* T:69 */
#define RDGAN_NHOURS 24        /* T:134 */
#define RDGAN_LOSS_SLOTS 8     /* floats appended behind the gradients in a gradient slab */

/* Build the per-(ndomain, max_batch) plans and allocate the activation workspace.
 * Replaces model construction at T:361-362 (create_generator / create_discriminator).
 * ndomain must be a multiple of 8 (L:324) from 8 to 120 -- fp32 storage runs all of them (the Dense kernel passes 4 GiB from
 * ndomain 104 on); the bf16 storage mode (rdgan_set_option "bf16") supports ndomain <= 72 and is refused above, with a message
 * in rdgan_last_error, when the option is set; n_cond_channels = 1 (T:129: the daily sum), 2 (+ longitude index,
 * revision1/additional_inputs/gan_train_cwgangp_pixelnorm_lon.py:136) or 3 (+ sin/cos day of year, …_doy.py:135):
 * every `cond` below is then [B,nd,nd,n_cond_channels], the generator's Dense has 100 + nd*nd*n_cond_channels
 * inputs and the critic's first Conv3D 1 + n_cond_channels input channels. */
int rdgan_create(rdgan_handle** out, int ndomain, int n_cond_channels, int max_batch);
void rdgan_destroy(rdgan_handle* h);
const char* rdgan_last_error(const rdgan_handle* h);
long rdgan_gen_param_count(const rdgan_handle* h);      /* 3 974 273 at ndomain 16 */
long rdgan_critic_param_count(const rdgan_handle* h);   /* 2 880 065 at ndomain 16 */
long rdgan_workspace_bytes(const rdgan_handle* h);

/* generator.predict([latent, cond]) (P:60, T:205,212; graph T:312-357).
 * z [B,100], cond [B,nd,nd,1] normalised daily sums -> out [B,24,nd,nd,1] hourly fractions. */
int rdgan_gen_forward(rdgan_handle* h, const float* gen_params, const float* z, const float* cond,
                      float* out, int B, void* stream);

/* tf.debugging.check_numerics(..., 'generator has nans or infs') behind the generator's softmax (T:349-350): waits for
 * `stream`, then returns -1 (and sets rdgan_last_error) if the generator output of the calls issued since the last
 * rdgan_gen_forward / rdgan_critic_grad / rdgan_gen_grad began contained NaN or Inf, else 0.  The gradient entries also
 * fold the same flag into slot 4 (nonfinite_flag) of their loss tail, so a training loop needs no extra sync (T:487-488). */
int rdgan_check_numerics(rdgan_handle* h, void* stream);

/* critic.predict([sample, cond]) (graph T:272-309).  seed == 0: dropout off (inference);
 * seed != 0: dropout masks of a train_on_batch pass (streams D1..D4 of rdgan_rng.h). out [B,1]. */
int rdgan_critic_forward(rdgan_handle* h, const float* critic_params, const float* sample,
                         const float* cond, float* out, int B, uint64_t seed, void* stream);

/* Gradient half of critic_model.train_on_batch([X_real, cond_real, latent], [valid, fake, dummy])
 * (T:472; graph T:363-392): generator forward (frozen), RandomWeightedAverage, three critic passes
 * as one 3B batch, the gradient-penalty double backward, loss = mean(-D(x)) + mean(D(G(z))) +
 * 10*mean((||grad_xhat D(xhat)||-1)^2).  grad_out[0:n_critic_params] = d loss / d critic weights,
 * grad_out[n .. n+8) = {total, valid, fake, gp, nonfinite_flag, 0, 0, 0}.  The caller all-reduces
 * grad_out over ranks (RCCL) and then calls rdgan_adam. */
int rdgan_critic_grad(rdgan_handle* h, const float* critic_params, const float* gen_params,
                      const float* x_real, const float* cond, const float* z, uint64_t seed,
                      float* grad_out, int B, void* stream);

/* The same, for callers that update the critic on another stream (data-parallel training: gradient all-reduce + Adam
 * on a communication stream).  The frozen generator's forward reads no critic weight, so it is issued first; `stream`
 * then waits for `critic_ready_event` (a hipEvent_t the caller recorded behind its last write of critic_params; NULL =
 * no wait) before the first kernel that reads critic_params.  The previous update thus overlaps the generator forward. */
int rdgan_critic_grad_after(rdgan_handle* h, const float* critic_params, const float* gen_params,
                            const float* x_real, const float* cond, const float* z, uint64_t seed,
                            float* grad_out, int B, void* critic_ready_event, void* stream);

/* rdgan_critic_grad_after for the LAST critic step of an iteration, told the batch of the generator step that follows it
 * (gen_z [gen_B,100], gen_cond [gen_B,nd,nd,1]; both NULL = rdgan_critic_grad_after).  With option "gen_fwd_ahead" on
 * (the default with fp32 storage) the call also issues that step's generator forward (gen_params), on a stream of the handle's own, forked right after the
 * critic input is built, so that it runs beside the rest of the critic step and whatever the caller issues next (its Adam).
 * The next rdgan_gen_grad(_after) on the handle with the same gen_params pointer and content version, z, cond pointers and
 * batch size skips its own forward and waits for that one instead: same kernels on the same data, results bit-identical to
 * the option off.  A different batch, pointer or version, or any other call on the handle first, drops it (the generator step
 * then runs its own forward).  The caller keeps gen_params, gen_z and gen_cond valid and unchanged until that generator step. */
int rdgan_critic_grad_ahead(rdgan_handle* h, const float* critic_params, const float* gen_params,
                            const float* x_real, const float* cond, const float* z, uint64_t seed,
                            float* grad_out, int B, void* critic_ready_event, const float* gen_z, const float* gen_cond,
                            int gen_B, void* stream);

/* Gradient half of generator_model.train_on_batch([latent, cond], valid) (T:482; graph T:395-408):
 * loss = mean(-D(G(z,c))), critic frozen, its dropout active.
 * grad_out[0:n_gen_params], grad_out[n .. n+8) = {loss, 0, 0, 0, nonfinite_flag, 0, 0, 0}. */
int rdgan_gen_grad(rdgan_handle* h, const float* critic_params, const float* gen_params,
                   const float* z, const float* cond, uint64_t seed, float* grad_out, int B,
                   void* stream);

/* rdgan_gen_grad with the same late wait for the critic weights (see rdgan_critic_grad_after): the generator forward
 * runs in front of it. */
int rdgan_gen_grad_after(rdgan_handle* h, const float* critic_params, const float* gen_params,
                         const float* z, const float* cond, uint64_t seed, float* grad_out, int B,
                         void* critic_ready_event, void* stream);

/* tf.optimizers.Adam(lr, beta_1=0, beta_2) apply step (T:385): v = b2 v + (1-b2) g^2,
 * p -= lr*sqrt(1-b2^t) * g / (sqrt(v)+eps), g = grad*grad_scale (1/world after the all-reduce sum).
 * t = the optimizer's shared iteration counter after increment (both models share it, T:391,408). */
int rdgan_adam(float* params, const float* grad, float* v, long n, int t, float lr, float beta2,
               float eps, float grad_scale, void* stream);

/* Weight-form cache.  Every gradient / forward entry first derives "weight forms" from the parameter slabs it is given
 * (generator: the transposed last kernel and the collapsed or shared-centre forms of the three block kernels, plus their bf16
 * images in the storage mode; critic: transposed kernels, padded / bf16 images) -- weight-only kernels that are wasted work
 * while a network is frozen: the generator across the n_critic critic steps of an iteration (T:468-476), the critic across
 * the generator step and the critic step that follows it (T:482, next T:472).  The caller may vouch for the CONTENT of the
 * slabs it passes: versions set here hold for the following calls, and a call whose (slab pointer, version, form options)
 * equal those the forms in the workspace were built from skips the rebuild.  A version is any non-zero number the caller
 * changes whenever it writes the slab (the trainer: a fresh number after every Adam update or checkpoint load); 0 = unknown,
 * always rebuild (the default, and what a caller that cannot vouch passes).  Results are bit-identical either way.
 * rdgan_form_builds: how many times each network's forms have been built by this handle (tests). */
int rdgan_set_weight_versions(rdgan_handle* h, uint64_t gen_version, uint64_t critic_version);
int rdgan_form_builds(const rdgan_handle* h, long* gen_builds, long* critic_builds);

/* Parameter slab layout: fills offsets[0..10) / sizes with the element offset and size of
 * {kernel,bias} x 5 layers in Keras weight order; returns the number of tensors (10). */
int rdgan_gen_param_layout(const rdgan_handle* h, long* offsets, long* sizes);
int rdgan_critic_param_layout(const rdgan_handle* h, long* offsets, long* sizes);

/* Options.  "collapse" (default 1): evaluate each generator block UpSampling3D(2)+Conv3D(3x3x3,'same')
 * (T:330-331) as 8 parity phases of 2x2x2 taps on the un-upsampled grid with pre-summed weights --
 * algebraically identical, 3.375x fewer FLOPs in forward, input gradient and weight gradient; only the
 * fp32 rounding of the pre-summed weights differs.  0 = the reference's direct 27-tap form.
 * "wave_specialized" (default 1): big GEMMs run the producer/consumer kernel (4 loader waves streaming tiles
 * into LDS by DMA, 4 compute waves issuing only ds_read + MFMA); 0 = the single-role kernel everywhere;
 * 2 = producer/consumer kernel for every eligible shape regardless of size (tests).
 * "ws_ksplit" (default 1): mid-size producer/consumer launches whose workgroup count would leave part of the 256 CUs
 * idle in the last round split their K loop over 2..8 workgroups (partials folded by a finish kernel, fixed order);
 * 0 = never, n > 1 = force n-way splits wherever the shape allows (tests).
 * "fast_fwd" / "fast_bwd" (default -1 = by storage mode: on with fp32 storage, off in the bf16 storage mode, where the matrix
 * pipe is 16x faster and the plain collapsed form -- one GEMM per block, no difference / plane-sum passes -- is quicker;
 * 1 / 0 force it; need "collapse" 1): generator blocks 2 and 3 (block inputs with >= 6 hour
 * planes) in the shared-centre form along the hour axis: out[2s] = S x[s] - W0 E[s], out[2s+1] = S x[s] + W2 E[s+1]
 * with E[j] = x[j] - x[j-1] and S = W0+W1+W2, so both outputs of a source position share the S x[s] product -- 48
 * instead of 64 tap products per position, algebraically identical.  Forward: T = S x once per output plane pair,
 * then the difference part adds T in its epilogue; backward: plane-pair sums of the output gradient feed the S part,
 * the gradient wrt E is folded back by the adjoint of the differencing.  0 = the 64-tap collapsed form.
 * "bf16" (default 0; needs "collapse" and "g9_direct" at 1; ndomain <= 72, refused above): the bf16 storage mode -- today's name
 * of the option introduced as "mfma_bf16" (next entry; the old name is still accepted and sets the same option).  Since then the
 * activations and activation gradients also live in the workspace as bf16 and the slab kernels listed below exist only in this mode.
 * "mfma_bf16" (default 0; needs the shared-centre form): mixed mode for BASELINE configs 3-5.  The forward,
 * input-gradient, second-sweep and weight-gradient GEMMs of generator blocks 1-3 and critic layers 2-4 read bf16
 * copies of their operands (weight forms stored [N][K]) and run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation;
 * every tensor the caller or another kernel sees, all gradients and the optimizer state stay fp32.  Results move by
 * bf16 rounding (2^-9 per operand), so it is NOT the mode the fp32 metric is measured in.
 * "g9_direct" (default 1): backward of the last generator conv (64 -> 1) straight from the 1-channel dlogits with the
 * neighbouring hour planes in LDS: weight gradient without the [rows][27] im2col matrix, input gradient fused with
 * block 3's PixelNorm+LeakyReLU backward (no intermediate gradient tensor).  Needs 4 (nd+2)^2 floats of LDS (nd <= 72);
 * 0 (and larger domains) = im2col + column GEMMs + separate PixelNorm backward.
 * "resident" (default 1; bf16 storage mode): the forward GEMMs of the shared-centre form whose tile holds whole source
 * planes keep the tile's source rows resident in LDS and stream only the weights (each source row is fetched once per
 * channel chunk instead of once per tap and chunk); same arithmetic in the same order, bit-identical to 0.
 * "upconv_slab" (default 1; bf16 storage mode, ndomain 16, collapsed form): the forward of generator block 3 (128 -> 64
 * channels onto the 24 x 16 x 16 grid, the dominant launch of the mode) runs in the slab kernel k_upconv_slab16: two source hour
 * planes + their halo resident in LDS for all 8 phases x 8 taps, weights streamed global -> VGPR in MFMA-fragment order, bias +
 * PixelNorm + LeakyReLU + bf16 rounding in registers (rdgan_upconv16.hip.h).  Same products as the streaming GEMM it replaces,
 * summed in another order: outputs agree to one bf16 ulp.  0 = the streaming GEMM (k_conv_gemm_ws<256, 64, ..., bf16>).
 * "upconv2_slab" (default 1; same conditions): the forward of generator block 2 (256 -> 128 channels onto the 12 x 8 x 8 grid) in the
 * slab kernel k_upconv2_slab16: a sample's whole block input (48 KB) resident in LDS for all 8 phases x 8 taps, the four waves of a
 * workgroup split the 128 output channels (each streams its own weight fragments) and exchange the PixelNorm row sums of squares
 * through LDS once per phase (rdgan_upconv16b.hip.h).  0 = the streaming GEMM (k_conv_gemm_ws<128, 128, ..., bf16>).
 * "g9_fused" (default 1; with "upconv_slab" and "tapgather"): the tap products of the generator's last Conv3D (64 -> 1, T:345) are
 * formed in the epilogue of the block-3 slab kernel from the rows it holds in registers (four more MFMAs per 32 rows) and summed over
 * (kh, kw) and the hour taps inside the work item; k_tapsum_softmax12 adds the source parity classes and the neighbouring items and
 * takes the softmax.  No pass over block 3's output (k_g9_fwd); a critic step does not store that output at all.  Same bf16 products
 * as 0, another fp32 summation order: fractions agree to ~3e-7 of the largest.
 * "upconv_slab_t" (default 1; bf16 storage mode, collapsed form, ndomain > 16 whose block-3 source planes are multiples of 8 x 8:
 * 32, 48, 64, ... -- the large-domain variant L:355-358): block 3 forward in the TILED slab kernel k_upconv_slab_t16: (h, w) tiles of
 * 8 x 8 source positions with their halo resident in LDS, the K loop in two channel halves (rdgan_upconv16t.hip.h); with "g9_fused"
 * the last conv's tap products leave its epilogue too, the tiles' edge sums as halo terms (k_g9_halo_fold, k_tapsum_softmax12t).
 * One bf16 ulp from the streaming GEMM; fractions within 2e-5 of the separate pass.
 * "conv_f16" (default 1; bf16 storage mode): the gather GEMMs with N % 128 == 0 and a bf16 destination that launch >= 640 workgroups
 * of 256 x 128 -- generator blocks 1 / 2 forward and input gradients, critic layers 2-4 forward and input gradients where no slab
 * kernel takes them -- by k_conv_gemm_f16 (rdgan_gemm_f16.hip.h): four waves and no loader waves, weights global -> VGPR from
 * fragment-order twin images (written beside the [tap][N][K] ones), gathered rows by LDS-DMA one 64-k chunk ahead, per-wave epilogue.
 * Same chunk and k order as the streaming kernel: bit-identical results except through a fused PixelNorm (one ulp of 1/l2).
 * 0 = k_conv_gemm_ws everywhere; 2 (tests) = regardless of the launch size.
 * "wgrad_wide" (default 0; bf16 storage mode): the streaming weight gradients of N % 128 == 0 layers with >= 32768 gathered rows on
 * 256 x 128 tiles with three LDS stages, one workgroup per CU (k_wgrad_gemm_ws16<256, 128>).  Correct and SLOWER (1.6-2x): kept for
 * the record and its tests.
 * "dense_skinny" (default 1; bf16 storage mode with "dense16", handles of max_batch <= 128): the Dense layer by k_dense16_skinny --
 * weights and input rows streamed in MFMA-fragment order, no LDS (the large domain's 415 MB kernel at 3.4-3.7 TB/s).  One bf16 ulp.
 * "wgrad_boxes" (default 1; with "border_boxes"): the weight gradients of critic layers 2-4 that run in the streaming kernels (fp32
 * storage: all three; bf16 storage: the layers without a slab kernel) use the border-class boxes too: per-phase tile and split
 * counts, one fold per weight tap over every phase that lists it (k_wgrad_reduce_box).  Same products, same results to ~1e-9.
 * ("d1_dgrad_fused" at ndomain > 16, multiples of 16: the same one-pass layer-1 input gradient on tiles of 24 x 16 x 8 input voxels,
 * k_d1_dgrad_tile16; bit-identical to the column GEMM + col2im.)
 * "d1_fwd_sample" (default 1; bf16 storage mode, ndomain 16, one condition channel): forward and second sweep of the critic's first
 * layer with a sample's input volume resident in LDS (k_d1_fwd_sample16); the second sweep then takes its gate from the 2-bit codes
 * ("d2_gate_bits"; without them it keeps the tile kernel).  One bf16 ulp from 0 in ~4e-5 of the activations.
 * "dense16" (default 1; bf16 storage mode): the generator's Dense layer on the bf16 matrix pipe: input rows and kernel rounded to
 * bf16, K padded to a multiple of 64, three launches of a third of the columns each (the streaming kernel wants N / 128 to be a power
 * of two).  0 = the fp32-pipe kernel with bf16 output.
 * "g9_bwd_mfma" (default 1; bf16 storage mode, collapsed backward): the input gradient of the generator's last conv + block 3's
 * PixelNorm backward on the fp32 matrix pipe (k_g9_bwd_mfma16: exact fp32 products); 0 = the VALU kernel k_g9_bwd_pairs.
 * "border_boxes" (default 1; 2 = at every size, 0 = off): the forward, second-sweep and input-gradient GEMMs of critic layers 2-4
 * (stride-2 'same' convs on 6x4x4 / 3x2x2 / 2x1x1 output grids) run on plans whose loop spaces are cut into border-class boxes,
 * each listing only the taps that can land inside the picture: 38 / 38 / 70 % fewer (row, tap) products at ndomain 16, all of them
 * products with a zero row.  Same products in the same tap order as the one-phase plans; small launches (few rows) keep the
 * one-phase plan, whose long K the K split needs.
 * "d2_gate_bits" (default 1; with "d2_slab" and the layer-1 edge kernels): the forward of layer 1 also writes its gate -- per element
 * LeakyReLU' = 1 or alpha, dropped or kept -- as 2 bits (16 bytes per row), and the slab kernel of layer 2's input gradient reads
 * that instead of layer 1's stored output (128 bytes per row): identical results.
 * "d2_fwd_slab" (default 0 -- measured no faster than the streaming GEMM, kept parity-tested; bf16 storage mode, ndomain 16): the forward of the critic's second layer in the slab kernel
 * k_d2_fwd_slab16: a sample's layer-1 output (69 KB) resident in LDS for all 27 taps, the four waves of a workgroup split the 128
 * output channels and stream their own weight fragments, bias + LeakyReLU + dropout in registers (rdgan_d2fwd16.hip.h); the
 * penalty's second sweep keeps the streaming GEMM.  Same dropout counter as 0 = k_conv_gemm_ws<128, 128, ..., bf16>.
 * ("d2_slab" at ndomain 32 / 48 / 64: k_d2_dgrad_slab_t16, the same on 8 x 8 tiles of destination positions of two samples.)
 * "d2_slab" (default 1; bf16 storage mode, ndomain 16): the input gradient of the critic's second layer (128 -> 64 channels onto
 * the 11 x 7 x 7 grid, eight parity phases of 8 ... 1 taps) runs in the slab kernel k_d2_dgrad_slab16: two samples' output
 * gradient resident in LDS for all phases and taps, weights streamed in MFMA-fragment order, LeakyReLU' x dropout gate + bf16
 * rounding in registers (rdgan_d2slab16.hip.h).  Same taps and k order as the streaming GEMM (0).
 * "d2_wgrad_slab" (default 1; bf16 storage mode, ndomain 16): the weight gradient of the critic's second layer runs in the slab
 * kernel k_d2_wgrad_slab16: a wave owns one of the 27 taps and keeps its 64 x 128 product in registers over the workgroup's share
 * of the batch; by input parity the taps fall into 8 classes, each a dense sub-grid of layer 1's output on which its taps are shifts
 * (rdgan_d2wgrad16.hip.h).  0 = k_wgrad_gemm_ws16<128,128>.  At ndomain 32 / 48 / 64 the same kernel body with work items = 4 x 4 tiles
 * of output positions and one halo position per odd class (k_d2_wgrad_slab_t16).
 * "d3_wgrad_slab" (default 1; same conditions): critic layer 3's weight gradient the same way (k_d3_wgrad_slab16: a wave owns a tap
 * and a quarter of the 256 output channels; a sample has 12 output positions, so an item is four samples); 0 = k_wgrad_gemm_ws16.
 * "upwgrad_slab" (default 1; bf16 storage mode, ndomain 16, collapsed form): the weight gradient of generator block 3 runs in the slab
 * kernel k_upconv_wgrad_slab16: a workgroup owns one output-parity phase and keeps its eight tap products (eight 128 x 64 fp32
 * tiles, one per wave) in registers over its share of the batch; source planes and output-gradient rows arrive by LDS-DMA in two
 * stages, both MFMA operands are read transposed from the position-major images (rdgan_upwgrad16.hip.h); block 2 the same way with a
 * workgroup per (phase, quarter of the 256 input channels) (k_upconv2_wgrad_slab16).  Both deliver the block's bias gradient from
 * the output-gradient fragments they multiply.  0 = k_wgrad_gemm_ws16 + column-sum passes.
 * "d1_dgrad_fused" (default 1; bf16 storage mode, ndomain 16, one condition channel): the first critic layer's input gradient
 * with respect to the sample channel (the penalty's dD/dx_hat and the generator step's dL/dfake) in one pass per sample
 * (k_d1_dgrad_sample16: the 539 x 27 tap products of a sample stay in LDS, the outputs gather from there); same sums in the same
 * order as 0 = column GEMM [rows][64] in HBM + k_d1_col2im.  fp32 storage, ndomain 16: the same by k_d1_dgrad_sample32 on the fp32
 * matrix pipe (the k order of the streaming GEMM: the same products); in the critic step's gradient-penalty sweep that pass also
 * takes the per-sample norm, the penalty term and the second sweep's input (k_gp_norm_r0's work, same reduction order): 0 = the
 * column GEMM + k_d1_col2im + k_gp_norm_r0.  Other ndomains with fp32 storage keep the column GEMM.
 * "combine_dx_fused" (default 1; fp32 storage, shared-centre backward "fast_bwd"): the gradient of a block's difference part is
 * folded into the block's input gradient by the PixelNorm/LeakyReLU backward of the block before it (k_pn_lrelu_bwd_pairs /
 * k_pn_lrelu_bwd form dx + (dE[d] - dE[d+1]) per element, k_combine_dx's expression; the combined dx is not stored: nothing else
 * reads it).  0 = k_combine_dx in a pass of its own.  Bit-identical either way.
 * "d1_wgrad16" (default 1; bf16 storage mode, one condition channel): the first critic layer's weight gradient runs on the bf16
 * matrix pipe (k_d1_wgrad16: im2col rows rounded to bf16 as in the layer's forward GEMM, both operands read transposed from
 * position-major LDS images) and delivers the layer's bias gradient from a ones column of the same product; 0 = the fp32-pipe
 * kernel k_d1_gemm_wgrad<bf16> + a column-sum pass.
 * "edge_kernels" (default 1): the weight gradient of the generator's last conv (64 -> 1) runs on the matrix pipe with the block-3
 * output streamed once (k_g9_wgrad_mfma; ndomain a power of two, otherwise the scalar kernel); the first critic layer (2 -> 64
 * channels, K = 54; one condition channel) runs as one K = 64 GEMM
 * per 128-row tile -- forward, the penalty's second sweep and the weight gradient (rdgan_edge.hip.h) -- instead of nine K
 * chunks of the tiled kernel; and in the bf16 storage mode the generator's last conv (64 -> 1) runs in its dedicated streaming
 * kernel (one pass over the block-3 output at HBM speed, same arithmetic and tap-sum format as "tapgather"); 2 = also with
 * fp32 storage (bit-identical to the tiled GEMM, not faster there); 0 = the tiled GEMM kernel everywhere.
 * "dense_wgrad_slices" (default 0 = by batch size; tests): row slices of the critic Dense weight gradient (1..16).
 * "split3" (default 0; optional data point, not the BASELINE metric): with fp32 storage, the forward / input-gradient conv GEMMs
 * of the producer/consumer kernel multiply on the bf16 matrix pipe -- every fp32 operand is split in registers into three bf16
 * parts (x = x1 + x2 + x3, 24 significant bits) and a product is the sum of six partial products, accumulated in fp32.  Memory,
 * LDS images, epilogues and the weight-gradient kernels are those of the fp32 path; errors against the fp64 oracle stay within
 * the fp32 path's tolerances (observed 1-3x its error).
 * "side_stream" (default 1): inside a call the weight-only kernels (generator weight forms, critic weight transposes and
 * bf16 images) and the bias-gradient column sums are issued on a second stream owned by the handle, beside the GEMMs on the
 * caller's stream and ordered against it by events (fork at entry, joins in front of the first reader / at the end of the
 * call): ~50 launches of 5-30 us per iteration leave the critical path.  The call's contract is unchanged (everything is
 * complete when `stream` is); same kernels on the same data, results bit-identical to 0.
 * "gen_fwd_ahead" (default -1 = by storage mode: on with fp32 storage, off in the bf16 mode): rdgan_critic_grad_ahead issues the
 * next generator step's forward beside the critic step's tail (see there); 0 = that call is rdgan_critic_grad_after, the schedule
 * of the entries without the generator batch; 1 = on in both modes.
 * "sample_offset" (default 0): global index of this rank's first sample.  RandomWeightedAverage's alpha (T:222-223) of
 * local sample k is uniform(key(seed, ALPHA), sample_offset + k), so ranks that share a seed draw the alphas of the
 * global batch (used by the data-parallel equivalence tests; the dropout masks stay keyed by the local element index).
 * "keep_gates" (default 0; test hook): a critic step keeps a copy of the interpolated third of its activations before the
 * penalty's second sweep overwrites it in place, so that rdgan_debug_activation returns the LeakyReLU / dropout pattern of all
 * 3B samples; allocates its buffers when set (not inside a step).
 * "tapgather" (default 1): the last generator conv (64 -> 1, T:345) runs as a column GEMM over its 27 taps whose
 * epilogue already sums the taps that fall inside the 256-row tile (ndomain 8/16: whole planes, 32/64/128: whole
 * rows), writing 3 or 9 floats per grid point instead of 32; 0 (and every other ndomain) = full column matrix +
 * separate gather kernel. */
int rdgan_set_option(rdgan_handle* h, const char* name, int value);

/* Per-kernel HIP-event timing for bench.py's roofline line.  tag_mask: bit i enables timing of
 * kernel class i (RDGAN_TAG_*).  rdgan_profile_read synchronises the device. */
enum {
  RDGAN_TAG_GCONV_FWD = 0,   /* fused upsample+Conv3D forward GEMMs of the generator */
  RDGAN_TAG_GCONV_DGRAD = 1,
  RDGAN_TAG_GCONV_WGRAD = 2,
  RDGAN_TAG_CRITIC_GEMM = 3,
  RDGAN_TAG_ELEMENTWISE = 4,
  RDGAN_TAG_GCONV3_FWD = 5,  /* the single dominant launch: forward of the 128->64 block at 24x16x16 (its difference part in the shared-centre form) */
  RDGAN_NUM_TAGS = 8
};
int rdgan_profile(rdgan_handle* h, unsigned tag_mask);
/* Algorithmic FLOPs (2 * rows * taps * K * N, of the algebraic forms actually run: collapsed / shared-centre) of every GEMM
 * this handle has launched since the last reset -- the numerator of bench.py's whole-iteration roofline fraction. */
int rdgan_flop_count(rdgan_handle* h, double* flops, int reset);
int rdgan_profile_read(rdgan_handle* h, int tag, double* total_ms, long* launches);
/* Per-launch table for bench.py's `roofline.launches`: with rdgan_profile_launches(h, 1) every GEMM launch (conv / input-gradient /
 * weight-gradient plans and the dedicated first- and last-layer kernels) is bracketed by HIP events on its launch stream and
 * recorded with its plan, kernel tile, batch and algorithmic FLOPs (2 * rows * taps * K * N of the form actually run; a launch
 * with split K includes its finish kernel, a weight gradient its partial-slab fold).  rdgan_launch_table synchronises the
 * device and returns one row per (plan, kind, batch, kernel): launches, summed GFLOP and summed milliseconds since the
 * recording was switched on.  kind: 0 = forward-type GEMM over the plan, 1 = weight gradient, 2 = dedicated edge kernel. */
typedef struct {
  int plan, kind, batch, launches;
  double gflop, ms;
  char name[48];       /* what the plan computes, e.g. "gen block3 fwd difference part" */
  char kernel[48];     /* kernel and tile, e.g. "k_conv_gemm_ws<256,64,TG4>" */
} rdgan_launch_stat;
int rdgan_profile_launches(rdgan_handle* h, int on);
int rdgan_launch_table(rdgan_handle* h, rdgan_launch_stat* out, int cap, int* n_out);

/* Input pipeline either side of the step (device-resident radar array data[n_days][24][ny][nx], fp32).
 * rdgan_data_gather: the tile gather + normalisation of generate_real_samples / generate_latent_points
 * (T:149-166, T:181-190): indices[n][3] = (tidx, yidx, xidx) int32 on the device; batch_out [n,24,nd,nd,1] =
 * hourly fractions of the daily sum (NULL: condition only), cond_out [n,nd,nd,1] = daily sum / norm_scale;
 * *flags |= 1 for a non-finite value (the reference asserts none, T:169-170), |= 2 for a finite fraction outside [0,1]
 * (T:171-172; with batch_out NULL only bit 1, for the condition).  The word ACCUMULATES: rdgan_data_gather never clears it, so one
 * read after several gathers sees all of them.  The caller owns it: it zeroes the word before the first gather and again after it
 * has read it (DeviceDataset.check_flags does both).  -2 = bad argument (NULL data / indices / cond_out / flags, non-positive
 * n_days / n / ndomain, ndomain > ny or > nx); the indices themselves are not checked on the device (DeviceDataset.set_indices does).
 * rdgan_data_valid_tiles: compute_valid_indices.py:74-92 -- valid_out[day][ii/stride][jj/stride] (int32 0/1) for the
 * boxes ii in range(0, ny-ndomain, stride), jj in range(0, nx-ndomain, stride): no NaN in the daily sum and at
 * least n_thresh points above tp_thresh_daily.  Bit-identical to the numpy forms.  rdgan_data_valid_tiles takes at most 2^24 - 1
 * boxes per call (-2 beyond: one workgroup per box; rdgan_data_valid_tiles_daily has no such limit); -2 also for a NULL pointer,
 * non-positive extents, stride < 1 and ndomain > ny or > nx.  No boxes (ny == ndomain, say) is success and writes nothing. */
int rdgan_data_gather(const float* data, int n_days, int ny, int nx, const int* indices, int n, int ndomain,
                      float norm_scale, float* batch_out, float* cond_out, int* flags, void* stream);
int rdgan_data_valid_tiles(const float* data, int n_days, int ny, int nx, int ndomain, int stride,
                           float tp_thresh_daily, int n_thresh, int* valid_out, void* stream);

/* Training set from raw radar frames: the host scripts in front of everything above, on the device.
 * rdgan_data_radar_hourly: convert_smhi_radardata.py:38-44 and reformat_data.py:72-91.  codes [n_days][24 * frames_per_hour][ny][nx]
 * uint8 radar codes (device, contiguous); lut256 [256] floats (device): the value of each code per frame, NaN at the missing code
 * (data_pipeline.radar_lut evaluates the reference's formula in its operation order).  hourly_out [n_days][24][ny][nx] =
 * ((lut[c0] + lut[c1]) + lut[c2]) + ... over the frames of the hour in order, fp32 -- one missing frame makes the hour NaN
 * (skipna=False); daily_out [n_days][ny][nx] (NULL: not wanted) = the sequential fp32 sum of the 24 rounded hourly values;
 * *missing_out (NULL: not wanted) is INCREASED by the number of NaN values written to hourly_out: the caller zeroes it, calls over
 * ranges of days add up.  frames_per_hour is one of 1, 2, 3, 4, 6, 12.  Any alignment of codes is accepted (16 codes per lane when
 * ny * nx is a multiple of 16 and the pointers are 16-byte aligned, 4 when a multiple of 4, else bytes); indexing is 64-bit.
 * rdgan_data_daily_sum: daily_out [n_days][ny][nx] of an hourly array that came from elsewhere, the same sequential sum
 * (np.sum(data[tidx], axis=0) of compute_valid_indices.py:81).
 * rdgan_data_valid_tiles_daily: the box test of compute_valid_indices.py:83-91 on that plane -- valid_out as
 * rdgan_data_valid_tiles writes it, for any stride >= 1, reading 1 float per pixel of a box instead of 24.
 * All three: asynchronous on the stream, 0 = success, -2 = bad argument (frames_per_hour not in the list, non-positive extents,
 * ndomain > ny or > nx). */
int rdgan_data_radar_hourly(const unsigned char* codes, const float* lut256, long n_days, int frames_per_hour, int ny, int nx,
                            float* hourly_out, float* daily_out, unsigned long long* missing_out, void* stream);
int rdgan_data_daily_sum(const float* hourly, long n_days, int ny, int nx, float* daily_out, void* stream);
int rdgan_data_valid_tiles_daily(const float* daily, long n_days, int ny, int nx, int ndomain, int stride, float tp_thresh_daily,
                                 int n_thresh, int* valid_out, void* stream);

/* Ensemble CRPS per grid point, properscoring.crps_ensemble(obs, ens, axis=0) of generate_and_evaluate_crps.py:188:
 * ens [n][npix] (member-major), obs [npix], optional scale [npix] applied to the members first (fractions -> mm/h,
 * :186), crps_out [npix] = mean|x_i - y| - 0.5 mean|x_i - x_j|.  n <= 8192. */
int rdgan_crps_ensemble(const float* ens, const float* obs, const float* scale, float* crps_out, int n, long npix,
                        void* stream);

/* The "random" climatological baseline of generate_and_evaluate_crps.py:164, 193-194: properscoring.crps_ensemble(real_precip,
 * baseline, axis=0) for MANY days against ONE ensemble.  ens [n][24][nd][nd] (finite values), obs [n_days][24][nd][nd];
 * crps_out [n_days][24][nd][nd] = mean|x_i - y| - 0.5 mean|x_i - x_j| per grid point, hourly_out [n_days][24] its area mean
 * (:194); either may be NULL, not both.  The members of a grid point are sorted once per call and every day costs a binary search
 * (fp64 prefix sums, results rounded to fp32); the area mean is an fp64 sum in a fixed order: repeated calls agree bit for bit.
 * A NaN observation gives NaN at its grid point and in its hour's mean.  1 <= n <= 8192, n_days * 24 nd^2 < 2^31. */
int rdgan_crps_fixed_ensemble(const float* ens, const float* obs, float* crps_out, float* hourly_out, int n, long n_days, int nd,
                              void* stream);
/* analyze_crps_results.py:25-35, the resampled means of bootstrapped_difference_onesample: means_out [n_resamples], entry j the
 * mean of n draws x[idx] for resample r = first_resample + j, idx = (uint64(rd_bits(rd_member_key(rd_make_key(seed,
 * RD_STREAM_BOOTSTRAP), r), i)) * n) >> 32 for draw i = 0 .. n - 1 (rdgan_rng.h; the reference draws np.random.choice).  A value
 * depends on (seed, r) only; fp64 sums in a fixed order.  n < 2^32, n_resamples < 2^31. */
int rdgan_bootstrap_means(const double* x, long n, uint64_t seed, long first_resample, long n_resamples, double* means_out,
                          void* stream);
/* The moments behind scipy.stats.ttest_1samp of analyze_crps_results.py:14: out3 = { n, mean, variance with ddof = 1 } of x [n] in
 * fp64, two passes, fixed order. */
int rdgan_moments_f64(const double* x, long n, double* out3, void* stream);

/* Distribution checks, generate_and_evaluate.py:431-604.  Samples lie as the reference holds them: x [batch][n][ncol], a column
 * being the n values of one (batch, col) (ncol = 24 hours in every reference use).  One workgroup per column; the column is sorted
 * once in LDS, hence 1 <= n <= 16384 (-2 beyond).  All three are asynchronous on `stream`, allocate nothing, take fp64 sums in a
 * fixed order and use no floating-point atomics: repeated calls agree bit for bit.
 *
 * rdgan_ks_2samp: the statistic of scipy.stats.ks_2samp(a_col, b_col) of :583, two-sided.  a [batch][n][ncol], b [batch][m][ncol];
 * counts_out [batch][ncol][2] = (i, j) = (#{a <= v}, #{b <= v}) at the first data value v where |i / n - j / m| is largest (both
 * ECDFs counted with <=, so equal values within or across the samples are all consumed before the difference is taken; "largest"
 * is decided on the integer |i m - j n|), d_out [batch][ncol] = fabs((double)i / n - (double)j / m); for n = m, |i - j| / n
 * exactly.  A column holding a NaN in either sample: counts (-1, -1), d NaN.  1 <= n, m <= 16384, batch * ncol < 2^31. */
int rdgan_ks_2samp(const float* a, const float* b, int n, int m, int ncol, long batch, int* counts_out, double* d_out,
                   void* stream);
/* matplotlib.cbook.boxplot_stats(x_col, whis=1.5), what sns.boxplot draws at :495, :499 and :600.  stats_out [batch][ncol][12]
 * doubles: n, mean, q1, med, q3, iqr, whislo, whishi, cilo, cihi, n_fliers_lo, n_fliers_hi.  Quartiles as np.percentile(x, [25,
 * 50, 75]) (linear, numpy's lerp, fp64, not contracted); whishi the largest datum <= q3 + 1.5 iqr (q3 if none at or above q3),
 * whislo the smallest >= q1 - 1.5 iqr (q1 likewise); cilo / cihi = med -/+ 1.57 iqr / sqrt(n); the fliers are the data outside
 * [whislo, whishi].  sorted_out (may be NULL) [batch][n][ncol]: the ascending column, whose first n_fliers_lo and last n_fliers_hi
 * entries are the fliers.  A column holding a NaN: n, then NaN in the other eleven slots and throughout its sorted column. */
int rdgan_box_stats(const float* x, int n, int ncol, long batch, double* stats_out, float* sorted_out, void* stream);
/* The ECDF of :431-435, :451-452 counted on thresholds, for any number of values in one pass.  grid [n_grid] ascending,
 * 1 <= n_grid <= 4096 (an unsorted grid is the caller's error and is not detected); x [n_values], 4-byte aligned,
 * 1 <= n_values <= 2^40.  counts_out [n_grid + 2] 64-bit integers: counts[j] = #{x <= grid[j]} exactly for j < n_grid, then the
 * number of values above the last threshold, then the number of NaNs (which belong to no threshold).  workspace: at least
 * rdgan_ecdf_workspace_bytes(n_grid) bytes of device memory (-2 for an n_grid outside 1..4096), cleared by the call.  Integer
 * atomics only, so the counts do not depend on the order of execution. */
long rdgan_ecdf_workspace_bytes(int n_grid);
int rdgan_ecdf_grid(const float* x, long n_values, const float* grid, int n_grid, long long* counts_out, void* workspace,
                    long workspace_bytes, void* stream);

/* Whole daily fields through the generator: the tiling and stitching around rdgan_gen_forward.
 * daily [n_days][ny][nx] fp32 on the device, mm/day.  Tile plan, the same in all three entries: nd = the generator's ndomain (one
 * rdgan_create accepts), 0 <= overlap <= nd / 2, ny >= nd, nx >= nd; step = nd - overlap; along an axis of length L the tiles start
 * at min(i * step, L - nd), i = 0 .. ceil((L - nd) / step); tile = iy * n_tx + ix, T = n_ty * n_tx tiles per day, n_days * T < 2^31.
 * All three: asynchronous on the stream (a host table is copied before the call returns), 0 = success, -2 = bad argument -- a null
 * pointer, an nd rdgan_create refuses, an overlap outside 0 .. nd / 2, ny or nx < nd, a count < 1, an entry or slot out of range --
 * and nothing is launched on a bad argument.
 *
 * rdgan_field_scan: counts_out [n_days][T][3] int32 (device) = per (day, tile) the number of wet pixels (finite and > 0), of NaN
 * pixels and of bad ones (negative or infinite).
 * rdgan_field_cond: the condition batch of m tiles.  entries [m] int32 on the HOST, entries[i] = day * T + tile, each in
 * 0 .. n_days * T - 1; cond_out [m][nd][nd][1] (device) = (float)((double)daily / norm_scale) -- the quotient
 * raindisagg_gan_pretrained.generate_scenarios forms -- and 0 where daily is NaN.  norm_scale > 0.
 * rdgan_field_blend: a group of `units` whole (scenario, day) units.  frac [m][24][nd][nd] (device), the output of rdgan_gen_forward
 * as it stands, m < 2^31; slots [units][T] int32 on the HOST: the row of frac that holds (unit, tile), -1 for a tile that was
 * skipped, every other value in 0 .. m - 1; unit u of the group is day (first_unit + u) % n_days, first_unit >= 0; ytab_idx [ny][3]
 * int32 and ytab_w [ny][3] fp32 (device): the (up to 3) tiles along y that cover a row, ascending, -1 when there are fewer, and
 * their weights, which sum to 1; xtab_idx [nx][3], xtab_w likewise; out [units][24][ny][nx] (device), any 4-byte alignment:
 *   out[u][h][y][x] = daily[day][y][x] * sum_a sum_b (ytab_w[y][a] * xtab_w[x][b]) * frac[slot][h][y - oy][x - ox]
 * in fp32, a outer and b inner, the products rounded before they are added; a skipped tile adds nothing; where daily is 0 the 24
 * values are 0 and where it is NaN they are NaN, whatever frac holds.  A table entry that does not cover its coordinate is ignored.
 * All offsets are 64-bit.  No atomics: repeated calls agree bit for bit. */
int rdgan_field_scan(const float* daily, long n_days, int ny, int nx, int nd, int overlap, int* counts_out, void* stream);
int rdgan_field_cond(const float* daily, long n_days, int ny, int nx, int nd, int overlap, const int* entries, long m,
                     double norm_scale, float* cond_out, void* stream);
int rdgan_field_blend(const float* frac, long m, const int* slots, long units, long first_unit, const int* ytab_idx,
                      const float* ytab_w, const int* xtab_idx, const float* xtab_w, const float* daily, long n_days, int ny, int nx,
                      int nd, int overlap, float* out, void* stream);

/* Ensemble products of whole fields.  All three: asynchronous on the stream, 0 = success, -2 = bad argument
 * (a null pointer, a bad shape, window list, probability, threshold, member count, stride or slot) with nothing launched and no
 * output touched; no floating-point atomics, repeated calls agree bit for bit; all offsets are 64-bit.
 *
 * rdgan_hourly_peaks: hourly [units][24][ny][nx] fp32 (device): scenarios of rdgan_field_blend, observed days, RainFARM members.
 * windows [n_windows] int32 on the HOST, strictly increasing, each in 1 .. 24, 1 <= n_windows <= 8.  With v the 24 hours of a pixel:
 *   peaks_out[u][i][y][x] = max over h0 = 0 .. 24 - windows[i] of v[h0] + v[h0 + 1] + .. + v[h0 + windows[i] - 1]
 * the sum taken in fp32 from left to right, every add rounded (no FMA), the maximum taken with `>` from h0 = 0 on;
 * peak_hour_out[u][y][x] (uint8) = the first h0 that reaches the maximum of windows[0].  A pixel with a NaN in any of its 24 hours
 * gives NaN for every window and hour 255.  peaks_out [units][n_windows][ny][nx] fp32, peak_hour_out [units][ny][nx] (device).
 * rdgan_field_blend_peaks: the arguments of rdgan_field_blend with the window list and the two outputs of rdgan_hourly_peaks in
 * place of `out`.  The hourly values are the ones rdgan_field_blend forms (same cover resolution, same order of products and adds)
 * and are reduced in registers: the result equals rdgan_hourly_peaks of rdgan_field_blend's output bit for bit, and the 24 hourly
 * planes are never written.  Where daily is 0 the peaks are 0 and the hour 0, where it is NaN they are NaN and 255, whatever frac
 * holds.
 * rdgan_member_stats: statistics across the members of an ensemble at every position.  x[s * member_stride + p] fp32 (device),
 * s < n_members (1 .. 4096), p < n_positions (1 .. 2^40), member_stride >= n_positions.  probs [n_probs] doubles on the HOST,
 * 1 <= n_probs <= 16, each in [0, 1]; thresholds [n_thresholds] doubles on the HOST, 0 <= n_thresholds <= 16, each finite
 * (thresholds and exceed_out may be NULL for 0).  Per position, over its n_members values:
 *   quantiles_out[q][p] = (float) np.quantile(x, probs[q], method="linear") -- virtual index (n - 1) q, numpy's lerp, fp64;
 *   mean_out[p]         = (float) (fp64 sum in a fixed order / n_members);
 *   exceed_out[t][p]    = (float) ((double) #{x > thresholds[t]} / n_members).
 * A position where any member is NaN gives NaN in every output; n_nan_positions_out (device, one 64-bit integer, cleared by the
 * call) counts those positions.  A workgroup sorts a run of adjacent positions side by side in LDS -- 64 positions up to 512
 * members, 32 up to 1024, 16 up to 2048, 8 up to 4096 -- so member rows are read in contiguous segments of that many floats. */
int rdgan_hourly_peaks(const float* hourly, long units, int ny, int nx, const int* windows, int n_windows, float* peaks_out,
                       unsigned char* peak_hour_out, void* stream);
int rdgan_field_blend_peaks(const float* frac, long m, const int* slots, long units, long first_unit, const int* ytab_idx,
                            const float* ytab_w, const int* xtab_idx, const float* xtab_w, const float* daily, long n_days, int ny,
                            int nx, int nd, int overlap, const int* windows, int n_windows, float* peaks_out,
                            unsigned char* peak_hour_out, void* stream);
int rdgan_member_stats(const float* x, int n_members, long member_stride, long n_positions, const double* probs, int n_probs,
                       const double* thresholds, int n_thresholds, float* quantiles_out, float* mean_out, float* exceed_out,
                       long long* n_nan_positions_out, void* stream);

/* Verification of field ensembles against the observed hours: rank histogram, Brier sums with the
 * reliability table, fractions skill score.  Positions p < n_positions are laid out ([D,] 24, ny, nx): the hour of p is
 * (p / (ny nx)) % 24.  thresholds [n_thresholds] doubles on the HOST, 1 <= n_thresholds <= 8, each rounded once to fp32 and compared
 * in fp32; finite, >= 0 and strictly increasing after the rounding.  n_members S in 1 .. 4096.  All four: asynchronous on the
 * stream, 0 = success, -2 = bad argument (a null pointer, a count, n_bins or threshold list out of range, an even or unsorted
 * width, S w^2 >= 2^26, a stride below n_positions, a workspace too small) with nothing launched and no output touched; every
 * accumulated value is an integer (the FSS sums: fp64 sums of integers in a fixed order, no floating-point atomics), so the results
 * do not depend on how the members are split into calls and repeated calls agree bit for bit; all offsets are 64-bit.
 *
 * rdgan_verify_accumulate: members[s * member_stride + p] fp32 (device), s < n_members of THIS call, member_stride >= n_positions
 * (1 .. 2^40); obs [n_positions] fp32.  Adds to the state (device, zeroed by the caller before the first call):
 *   exceed[t][p] += #{s : x_s[p] > thresholds[t]},  below[p] += #{s : x_s[p] < obs[p]},  equal[p] += #{s : x_s[p] == obs[p]}  (int32)
 *   bad[p] |= obs[p] is NaN or a member is NaN at p                                                                        (uint8)
 * IEEE comparisons: a NaN counts nowhere.  16-byte loads when the pointers are 16-byte aligned and member_stride and n_positions
 * are multiples of 4, a scalar path otherwise (4-byte alignment is required).  The caller keeps the total number of members <= 4096.
 * rdgan_verify_reduce: one pass over the state of S = n_members members in all; plane = ny nx, n_positions a multiple of plane (the last day may stop short of 24 hours).
 * Over the valid positions (bad == 0 and obs not NaN), per hour:
 *   rank = below + ((b24 (equal + 1)) >> 24) in 64 bits, b24 = rd_bits(rd_member_key(rd_make_key(seed, 8), p), 0) >> 8 (rdgan_rng.h):
 *   a tie among `equal` members and the observation is broken uniformly by a hash of (seed, p);
 *   rank_hist_out [24][S + 1] counts the ranks;
 *   with c = exceed[t][p], e = [obs[p] > thresholds[t]], bin = (c n_bins) / (S + 1), 2 <= n_bins <= min(S + 1, 64):
 *   reliability_out [T][24][n_bins][3] = (count, sum e, sum c) and brier_out [T][24][4] = (N, sum e, sum c e, sum c^2).
 * 64-bit integers (device), cleared by the call.
 * rdgan_verify_fss: per day, hour and threshold the planes C = exceed[t] and E = e, both 0 at a bad position; BC, BE their sums over
 * the w x w box centred at each pixel, clipped at the field's edge; at every pixel num += (BC - S BE)^2, den += BC^2 + (S BE)^2.
 * widths [n_widths] int32 on the HOST, 1 <= n_widths <= 8, odd, strictly increasing, S w^2 < 2^26.  fss_sums_out [T][W][24][2]
 * doubles (device) = (num, den) summed over days and pixels, cleared by the call; FSS = 1 - num / den.  Summed-area tables (a row
 * scan, a column scan, four reads per box): the cost per pixel does not grow with w^2.  workspace: at least
 * rdgan_verify_fss_workspace_bytes(ny, nx, n_thresholds, n_widths) bytes of device memory, 8-byte aligned (-2 from the sizing entry
 * for a count out of range); it holds one day's tables, whatever n_days is.  A state that holds more members than n_members (the
 * caller's error) is clamped to n_members by reduce and FSS alike, so every bound above holds whatever the state is. */
int rdgan_verify_accumulate(const float* members, int n_members, long member_stride, long n_positions, const float* obs,
                            const double* thresholds, int n_thresholds, int* exceed, int* below, int* equal, unsigned char* bad,
                            void* stream);
int rdgan_verify_reduce(const float* obs, const int* exceed, const int* below, const int* equal, const unsigned char* bad,
                        long n_positions, long plane, int n_members, const double* thresholds, int n_thresholds, int n_bins,
                        uint64_t seed, long long* rank_hist_out, long long* reliability_out, long long* brier_out, void* stream);
long rdgan_verify_fss_workspace_bytes(int ny, int nx, int n_thresholds, int n_widths);
int rdgan_verify_fss(const float* obs, const int* exceed, const unsigned char* bad, long n_days, int ny, int nx, int n_members,
                     const double* thresholds, int n_thresholds, const int* widths, int n_widths, double* fss_sums_out, void* workspace,
                     long workspace_bytes, void* stream);

/* Temporal structure of hourly fields: wet spells, transitions, wet hours per day, lagged products.
 * x [n][24][plane] fp32 (device), plane = ny nx, the leading axis with stride day_stride >= 24 plane (a view of a wider buffer is
 * accepted); leading axes -- days, or scenarios x days -- are flattened to n.  A series is one (i, q), i < n, q < plane: the 24
 * values x[h] = X[i day_stride + h plane + q].  Series are cut at the day boundary on purpose: generated days are independent of
 * each other, and observed days must be cut the same way to be comparable.  A series with a NaN or +-inf among its 24 hours is
 * bad: it adds 1 to n_bad and nothing else; n_valid counts the others.
 * thresholds [n_thresholds] doubles on the HOST, 1 <= n_thresholds = T <= 8, each rounded once to fp32 and compared in fp32;
 * finite, >= 0 and strictly increasing after the rounding.  Hour h is wet when x[h] > thr[t] (a value equal to the threshold is
 * dry); m is the 24-bit mask of wet hours.  A run is a maximal block of equal bits of m and never wraps round the day; its edge
 * class c is 1 if it contains hour 0 or hour 23 (it is cut off by the day boundary) and 0 otherwise.
 * counts_inout [T * 286 + 2] 64-bit integers (device), over the valid series; per threshold t, at t * 286 +
 *     0  wet_hours[k], k = 0 .. 24: series with popcount(m) = k
 *    25  longest_wet[k], k = 0 .. 24: series whose longest wet run has length k
 *    50  wet_spell[c][L - 1], c = 0, 1, L = 1 .. 24: wet runs of length L and edge class c
 *    98  dry_spell[c][L - 1]: the same for dry runs (a wholly dry day is one run with c = 1, L = 24)
 *   146  first_wet[h], h = 0 .. 23: series with a wet hour whose first wet hour is h
 *   170  last_wet[h]: the same for the last wet hour
 *   194  trans[h][a][b], h = 0 .. 22: series with wet(h) = a and wet(h + 1) = b
 * then n_valid at T * 286 and n_bad at T * 286 + 1.
 * sums_inout [48 + K + 24 T] doubles (device), over the valid series, K = max_lag in 1 .. 12:
 *     0  moments[h] = (sum x[h], sum x[h]^2), h = 0 .. 23
 *    48  lag[k - 1] = sum over series of sum_{h = 0}^{23 - k} x[h] x[h + k], k = 1 .. K
 *  48+K  wet_amount[t][h] = sum of x[h] over the valid series with hour h wet
 * every product formed exactly in fp64.  Both arrays ACCUMULATE over any number of calls; the caller zeroes them before the first.
 * The counts do not depend on how the series are split into calls or on the launch geometry (LDS counters merged with 64-bit
 * integer atomics).  The sums use no floating-point atomics: a fixed order in a thread, a fixed reduction in a workgroup, the
 * workgroups' partials added in order by a final kernel -- two identical sequences of calls agree bit for bit, and for
 * non-negative input a sum of N terms is within (N - 1) 2^-53 relative of the exact one in any grouping.
 * 16-byte loads when x is 16-byte aligned and plane and day_stride are multiples of 4, a scalar path otherwise (4-byte alignment
 * is required).  n * 24 * plane <= 2^40.  workspace: at least rdgan_temporal_workspace_bytes(n, plane, n_thresholds, max_lag)
 * bytes of device memory, 8-byte aligned (-2 from the sizing entry for an argument out of range).  Asynchronous on the stream;
 * 0 = success, -2 = bad argument (a null pointer, a misaligned pointer, n or plane < 1, a size above the limit, a threshold list
 * or max_lag out of range, day_stride < 24 plane, a workspace too small) with nothing launched and no output touched.  All
 * offsets are 64-bit. */
long rdgan_temporal_workspace_bytes(long n, long plane, int n_thresholds, int max_lag);
int rdgan_temporal_accumulate(const float* x, long n, long day_stride, long plane, const double* thresholds, int n_thresholds,
                              int max_lag, long long* counts_inout, double* sums_inout, void* workspace, long workspace_bytes,
                              void* stream);

/* Rain cells of hourly fields: the connected wet areas of every hour, labelled and counted.
 * x [n][24][ny][nx] fp32 (device), the leading axis with stride day_stride >= 24 ny nx (a view of a wider buffer is accepted);
 * leading axes -- days, or scenarios x days -- are flattened to n.  A plane is one (i, h), i < n, h < 24: ny nx values at
 * X[i day_stride + h ny nx + y nx + x].  ny nx <= 2^24 and n 24 ny nx <= 2^40.
 * thresholds [n_thresholds] doubles on the HOST, 1 <= n_thresholds = T <= 8, each rounded once to fp32 and compared in fp32;
 * finite, >= 0 and strictly increasing after the rounding.  A pixel is wet at threshold t when x > thr[t] (a value equal to the
 * threshold is dry).  A pixel that is NaN or +-inf is bad: never wet, and counted in n_bad_pixels.
 * A cell is a maximal set of wet pixels of ONE plane connected under `connectivity`, 4 (edges) or 8 (edges and corners); cells
 * never link across hours, days or scenarios.  The canonical label of a cell is the smallest flat index y nx + x among its
 * pixels; a pixel in no cell has label -1.  A cell has edge class c = 1 if it has a pixel in the first or last row or column of
 * the plane, or a bad pixel in the 8-neighbourhood of any of its pixels (the domain or the coverage cuts it off), else c = 0.
 * Per cell: area, its pixel count, and volume = sum of q(x), q(x) = rint(min(x, 2^20) 2^16) as a 64-bit integer -- the product is
 * exact in fp64, the rounding is half to even and happens once per pixel, so a volume does not depend on the order of the sum.
 * counts_inout [T * 317 + 2] 64-bit integers (device); per threshold t, at t * 317 +
 *     0  wet_pixels[h], h = 0 .. 23: wet pixels of the planes of hour h
 *    24  cells[c][h]: cells of edge class c in the planes of hour h
 *    72  area_hist[c][b], b = floor(log2(area)) = 0 .. 24: cells by area (bin 0 is exactly the single-pixel cells)
 *   122  area_sum[c]: the sum of the areas
 *   124  area_sq_sum[c]: the sum of the squared areas
 *   126  volume_by_area[c][b]: the sum of the volumes of the cells of bin b
 *   176  cells_per_plane[k], k = 0 .. 64: planes with k cells, the last bin open (64 or more)
 *   241  largest_area[b]: planes whose largest cell falls in bin b
 *   266  dry_planes: planes without a cell
 *   267  area_by_area[c][b]: the sum of the areas of the cells of bin b (volume_by_area over it is the bin's mean intensity)
 * then n_planes at T * 317 and n_bad_pixels at T * 317 + 1, once per state.  The array ACCUMULATES over any number of calls; the
 * caller zeroes it before the first.  Everything is an integer merged with integer atomics, so the state does not depend on how
 * the planes are split into calls, on the workspace size or on the launch geometry.  (The sums wrap modulo 2^64; area_sq_sum
 * reaches 2^63 only beyond 2^15 all-wet planes of 2^24 pixels.)
 * labels_out: null, or [n][24][ny][nx] int32 (device, dense): the canonical labels at threshold index label_threshold in 0 .. T-1.
 * workspace: device memory, 8-byte aligned.  rdgan_cells_workspace_bytes(ny, nx, planes_per_pass) is the size that lets a pass take
 * planes_per_pass planes (1 .. 65535; 16 bytes per pixel and 8 per plane; -2 for an argument out of range); the entry takes
 * floor(workspace_bytes / rdgan_cells_workspace_bytes(ny, nx, 1)) planes per pass, loops over the passes and the thresholds, and
 * the result does not depend on it.  Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n,
 * ny or nx < 1, a size above the limits, a threshold list out of range, connectivity not 4 or 8, label_threshold out of range
 * with labels_out given, day_stride < 24 ny nx, a workspace too small for one plane) with nothing launched and no output touched.
 * All offsets are 64-bit. */
long rdgan_cells_workspace_bytes(long ny, long nx, long planes_per_pass);
int rdgan_cells_accumulate(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                           int connectivity, long long* counts_inout, int* labels_out, int label_threshold, void* workspace,
                           long workspace_bytes, void* stream);

/* Object-based verification of hourly fields: the per-plane records from which SAL (Wernli, Paulat, Hagen
 * and Frei 2008) -- structure, amplitude, location -- of a generated plane against the observed one is formed on the host.
 * x, n, day_stride, ny, nx, thresholds, wet and bad pixels, connectivity: as for rdgan_cells_accumulate above; the objects of a
 * plane at threshold t are its cells there, with the same canonical labels.  The mass of a valid (finite) pixel is
 * q = (int) rintf(clamp(x, 0, 2048 - 1/1024) * 1024), 0 <= q < 2^21, in units of 2^-10 mm; its coordinates are the integers y, x.
 * plane_out [n * 24][4] 64-bit integers (device): n_bad, M0 = sum q, Mx = sum q x, My = sum q y over the valid pixels of the plane.
 * obj_out [n * 24][T][3] 64-bit integers (device): n_objects, n_wet, R = sum_n R_n, where for object n R_n = sum q, Rmax_n = max q,
 * Sx_n = sum q x, Sy_n = sum q y over its pixels.
 * vr_out [n * 24][T][2] doubles (device): V = (sum_n R_n (R_n / Rmax_n)) / R and
 * r = (sum_n R_n hypot(Sx_n / R_n - Mx / M0, Sy_n / R_n - My / M0)) / R, the sums over the objects with R_n > 0; both 0 when R = 0.
 * The outputs are OVERWRITTEN.  The integers are formed with integer atomics; the fp64 sums run over the objects in a tree fixed by
 * the pixel index of their labels and by ny nx alone, without floating-point atomics, so every record of a plane is bitwise the
 * same however the planes are split into calls or passes.
 * Every sum stays below 2^63 because a plane with 2^21 max(ny, nx) ny nx >= 2^63 is refused (on top of ny nx <= 2^24).
 * workspace: device memory, 8-byte aligned.  rdgan_sal_workspace_bytes(ny, nx, planes_per_pass) is the size that lets a pass take
 * planes_per_pass planes (1 .. 65535; 48 bytes per pixel, 40 per 4096 pixels begun and 200 per plane; -2 for an argument out of
 * range); the entry takes floor(workspace_bytes / rdgan_sal_workspace_bytes(ny, nx, 1)) planes per pass.  Asynchronous on the
 * stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n, ny or nx < 1, a size above the limits, a threshold list
 * out of range, connectivity not 4 or 8, day_stride < 24 ny nx, a workspace too small for one plane) with nothing launched and no
 * output touched.  All offsets are 64-bit. */
long rdgan_sal_workspace_bytes(long ny, long nx, long planes_per_pass);
int rdgan_sal_records(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                      int connectivity, long long* plane_out, long long* obj_out, double* vr_out, void* workspace,
                      long workspace_bytes, void* stream);

/* Scale-separation verification of hourly fields: the integer state of the intensity-scale skill score
 * (Casati, Ross and Stephenson 2004; Casati 2010) of s member arrays against the observed hours.
 * members [s][n_days][24][ny][nx] fp32 (device), member m at members + m * member_stride, member_stride >= n_days 24 ny nx;
 * obs [n_days][24][ny][nx] fp32 (device), dense.  1 <= s <= 4096, ny nx <= 2^24, s n_days 24 ny nx <= 2^40.
 * thresholds: 1 .. 8 values, as for rdgan_verify_accumulate; the event of a finite value v at threshold u is v > u in fp32.
 * levels = L, 1 .. 10, 2^L <= min(ny, nx): a tile is a square of side 2^L; the plane is cropped to floor(ny / 2^L) x
 * floor(nx / 2^L) tiles from (oy, ox) = ((ny mod 2^L) / 2, (nx mod 2^L) / 2), integer divisions.  A pair is one member plane
 * beside the observed plane of the same day and hour; a tile of a pair is void when any of its pixels is NaN or +-inf in the
 * member or in the observation, and then contributes nothing.
 * counts_inout, flat order [t][h][l][3], T x 24 x (L + 1) x 3 64-bit integers (device): summed over the blocks b of side 2^l
 * (aligned to the tile) of the valid tiles of all pairs of hour h, QX = sum SX_l(b)^2, QO = sum SO_l(b)^2, QXO = sum SX_l(b) SO_l(b),
 * SX and SO the events of the member and of the observation in b.  tiles_inout [h][2] 64-bit integers: (valid, void) tile-pairs.
 * Both are ADDED to with 64-bit integer atomics (the caller zeroes them before the first call), so the state does not depend on
 * how the members are split into calls, on the pass size or on the launch geometry.  One call adds at most
 * (pixel-pairs of the call) 4^L <= 2^40 2^20 = 2^60 to a counter; the caller keeps (pixel-pairs accumulated) 4^L <= 2^62.
 * workspace: device memory, 8-byte aligned.  rdgan_iss_workspace_bytes(ny, nx, levels, pairs_per_pass), pairs_per_pass 1 .. 2^30,
 * is the size that lets a pass hold that many pairs: 8 bytes a pair up to L = 6 (nothing is held), and for L = 7 .. 10
 * ceil(cy / 64) ceil(cx / 64) (8 x 4 x 20 x 4 + 8) bytes a pair, (cy, cx) the cropped size (-2 for an argument out of range).  The
 * entry takes floor(workspace_bytes / rdgan_iss_workspace_bytes(ny, nx, levels, 1)) pairs per pass.  Asynchronous on the stream;
 * 0 = success, -2 = bad argument (a null or misaligned pointer, a size < 1 or above the limits, levels outside 1 .. 10 or
 * 2^levels > min(ny, nx), a threshold list out of range, s > 4096, member_stride < n_days 24 ny nx, a workspace too small for one
 * pair) with nothing launched and no output touched.  All offsets are 64-bit. */
long rdgan_iss_workspace_bytes(long ny, long nx, int levels, long pairs_per_pass);
int rdgan_iss_accumulate(const float* members, int s, long member_stride, const float* obs, long n_days, long ny, long nx,
                         const double* thresholds, int n_thresholds, int levels, long long* counts_inout, long long* tiles_inout,
                         void* workspace, long workspace_bytes, void* stream);

/* Distance-map verification of hourly fields: the exact Euclidean distance transform of event sets and the
 * per-pair records from which Hausdorff distance, mean error distance, Baddeley's Delta and Zhu's measure are formed on the host.
 * For a threshold u (1 .. 8 values, as for rdgan_verify_accumulate) the set of a plane is its pixels with a finite value v > u in
 * fp32; a NaN or +-inf pixel is bad and in no set.  d2(x, S) = min over a in S of dy^2 + dx^2, an exact integer, measured in the
 * plane's own geometry across bad pixels; D(x, S) = isqrt(256 d2(x, S)) = floor(16 sqrt(d2)), the distance in 1/16 pixel, and
 * 0xFFFF for an empty S.  1 <= ny, nx <= 2048: D <= 46 318.
 * rdgan_dm_maps: x [n][24][ny][nx] fp32 (device), day i at x + i * day_stride, day_stride >= 24 ny nx, n 24 ny nx <= 2^40.
 * maps_out [n * 24][T][ny][nx] uint16 (device): D(x, S_t) of every plane and threshold; set_sizes_out [n * 24][T] 64-bit integers
 * (device): the pixels of each whole set.  Both are OVERWRITTEN.
 * rdgan_dm_records: members [s][n_days][24][ny][nx] fp32 (device), member m at members + m * member_stride, member_stride >=
 * n_days 24 ny nx, 1 <= s <= 4096, s n_days 24 ny nx <= 2^40; obs [n_days][24][ny][nx] fp32 (device), dense; obs_maps: the
 * maps_out of rdgan_dm_maps for obs and the same thresholds.  A pair is one member plane beside the observed plane of the same day
 * and hour; A is the member's set, B the observation's; a pixel is valid when it is finite on both sides.  cutoff16 = C, 16 ..
 * 65534, in 1/16 pixel: w(x, S) = min(D(x, S), C).  records_out [s][n_days * 24][T][12] 64-bit integers (device), OVERWRITTEN:
 *   0 n_valid; 1, 2, 3 nA, nB, nAB, the pixels of A, of B and of both among the valid ones;
 *   4 sum over valid x in B of D(x, A); 5 sum over valid x in A of D(x, B); 6, 7 the maxima of the same two (the directed Hausdorff
 *   distances); each of 4 .. 7 is 0 when the other set is empty;
 *   8, 9, 10 over valid x: sum |wA - wB|, sum (wA - wB)^2, max |wA - wB|;
 *   11 flags: bit 0 the bad-pixel masks of the two sides differ, bit 1 A empty, bit 2 B empty (the whole sets).
 * Every sum stays below 2^54 (2^22 pixels times 46 318^2).  Integer atomics only: the records are bitwise independent of how the
 * members are split into calls, of the pass size and of the launch geometry.
 * workspace: device memory, 8-byte aligned.  rdgan_dm_workspace_bytes(ny, nx, planes_per_pass), planes_per_pass 1 .. 2^20, is the
 * size that lets a pass take that many planes: 9 ny ceil(nx / 64) 8 + 64 bytes a plane (-2 for an argument out of range); the
 * entries take floor(workspace_bytes / rdgan_dm_workspace_bytes(ny, nx, 1)) planes per pass.  Asynchronous on the stream;
 * 0 = success, -2 = bad argument (a null or misaligned pointer, a size < 1 or above the limits, a side above 2048, a threshold
 * list out of range, s > 4096, a stride too small, cutoff16 out of range, a workspace too small for one plane) with nothing
 * launched and no output touched.  All offsets are 64-bit. */
long rdgan_dm_workspace_bytes(long ny, long nx, long planes_per_pass);
int rdgan_dm_maps(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                  unsigned short* maps_out, long long* set_sizes_out, void* workspace, long workspace_bytes, void* stream);
int rdgan_dm_records(const float* members, int s, long member_stride, const float* obs, const unsigned short* obs_maps, long n_days,
                     long ny, long nx, const double* thresholds, int n_thresholds, int cutoff16, long long* records_out,
                     void* workspace, long workspace_bytes, void* stream);

/* Storms of hourly fields: wet volumes connected through the day's hours, labelled and counted -- how long
 * a rain system lives, when it starts, and how much of the day's water falls in long-lived systems.
 * x, n, day_stride, ny, nx, thresholds, wet and bad pixels, connectivity, q(x): as for the cells entry above.  A voxel (h, y, x)
 * of day i has the day-local index v = h ny nx + y nx + x.  ny nx <= 2^24, 24 ny nx <= 2^27 and n 24 ny nx <= 2^40.
 * Two wet voxels of the SAME day are linked when they lie in the same hour and are neighbours under `connectivity` (exactly the
 * relation of the cells), or lie in consecutive hours h, h + 1 at pixels p, p + d with |dy|, |dx| <= reach, reach in 0 .. 4
 * (0: the plain overlap rule of cell tracking; 1: rain may move one pixel per hour).  A storm is a maximal set of wet voxels of
 * one day connected by links; days and scenarios never link.  Its canonical label is its smallest v; a voxel in no storm has
 * label -1.  Per storm: size, its voxel count (pixel-hours); volume = sum of q(x); start, the hour of its smallest v; last, its
 * largest hour; duration = last - start + 1 (links join consecutive hours only, so a storm's hours are contiguous).  Its class is
 * c = space_edge + 2 time_edge: space_edge if any of its voxels lies in the first or last row or column of the plane or has a bad
 * pixel in the 8-neighbourhood of its own hour (the edge flag of the cells); time_edge if start == 0 or last == 23 (the day
 * censors the duration).
 * counts_inout [T * 622 + 2] 64-bit integers (device); per threshold t, at t * 622 +
 *     0  wet_pixels[h], h = 0 .. 23: wet voxels of hour h
 *    24  storms[c], c = 0 .. 3: storms by class
 *    28  duration_hist[c][duration - 1]
 *   124  start_hour[c][start]
 *   220  size_hist[c][b], b = floor(log2(size)) = 0 .. 27
 *   332  size_sum[c]: the sum of the sizes
 *   336  size_sq_sum[c]: the sum of the squared sizes
 *   340  size_by_duration[c][duration - 1]: the sum of the sizes
 *   436  volume_by_duration[c][duration - 1]: the sum of the volumes
 *   532  storms_per_day[k], k = 0 .. 64: days with k storms, the last bin open (64 or more)
 *   597  longest_duration[k], k = 0 .. 24: days whose longest storm lasts k hours, k = 0 a day without a wet voxel
 * then n_days at T * 622 and n_bad_pixels at T * 622 + 1, once per state; the state-count entry returns T * 622 + 2, or -2 for T
 * outside 1 .. 8.  The array ACCUMULATES over any number of calls; the caller zeroes it before the first.  Everything is an
 * integer merged with integer atomics, so the state does not depend on how the days are split into calls, on the workspace size
 * or on the launch geometry.  (The sums wrap modulo 2^64; a volume sum of one day stays below 2^63.)
 * labels_out: null, or [n][24][ny][nx] int32 (device, dense): the canonical labels at threshold index label_threshold in 0 .. T-1.
 * workspace: device memory, 8-byte aligned.  The workspace-bytes entry gives the size that lets a pass take days_per_pass whole
 * days (1 .. 2730; 24 bytes per voxel, 8 per day and 8 per plane; -2 for an argument out of range); the accumulate entry takes as
 * many whole days per pass as the workspace holds, loops over the passes and the thresholds, and the result does not depend on it.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n, ny or nx < 1, a size above the
 * limits, a threshold list out of range, connectivity not 4 or 8, reach outside 0 .. 4, label_threshold out of range with
 * labels_out given, day_stride < 24 ny nx, a workspace too small for one day) with nothing launched and no output touched.  All
 * offsets are 64-bit. */
long rdgan_storms_state_count(int n_thresholds);
long rdgan_storms_workspace_bytes(long ny, long nx, long days_per_pass);
int rdgan_storms_accumulate(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                            int connectivity, int reach, long long* counts_inout, int* labels_out, int label_threshold,
                            void* workspace, long workspace_bytes, void* stream);

/* Areal extremes of hourly fields: depth-area-duration -- for every day the largest accumulation over any
 * k consecutive hours and any w x w box of pixels, and statistics of those maxima over the days.
 * x, n, day_stride, ny, nx and the size limits: as for rdgan_cells_accumulate above.  Everything is defined in integers:
 * q(x) = (int) rintf(x * 1024), in units of 2^-10 mm (the product is exact in fp32, the rounding is half to even).  A pixel-hour is
 * bad when x is NaN, +-inf, negative or >= 2048; so q < 2^21 and a box sum stays below 2^38.
 * windows [n_windows] ints on the HOST, 1 <= n_windows = K <= 8, strictly increasing in 1 .. 24 (as for rdgan_hourly_peaks).
 * widths [n_widths] ints on the HOST, 1 <= n_widths = W <= 8, strictly increasing in 1 .. 64, each <= min(ny, nx): boxes lie wholly
 * inside the plane and are never clipped.  levels [n_levels] doubles in mm on the HOST, 0 <= n_levels = L <= 16 (null for 0),
 * finite, strictly increasing, each in [0, 2048 * 24]; L_q[l] = llrint(levels[l] * 1024).
 * For day u, window k, width w, start hour h0 <= 24 - k and corner (y0, x0), A(h0, y0, x0) is the sum of q over the k hours from h0
 * and the w x w pixels from (y0, x0); a (window, box) that holds a bad pixel-hour is left out.  Amax[u][k][w] is the maximum of A over
 * what remains, h*[u][k][w] the smallest h0 that attains it; Amax1[u][k] is Amax at w = 1, computed whether or not 1 is a width.
 * counts_inout [K * W * (L + 53) + 2] 64-bit integers (device); the record of (k, w) lies at (k W + w) (L + 53) +
 *     0       level_count[b], b = 0 .. L: days by b = #{l : Amax >= L_q[l] w^2}
 *     L + 1   start_hour[h], h = 0 .. 23: days by h*
 *     L + 25  arf_hist[r], r = 0 .. 20: days by min(20, (20 Amax) / (w^2 Amax1)), integer division; only days with Amax1 > 0
 *     L + 46  sum_A: the sum of Amax over the days in arf_hist
 *     L + 47  sum_A1: the sum of Amax1 over the same days (the pooled areal reduction factor is sum_A / (w^2 sum_A1))
 *     L + 48  sum_A_all: the sum of Amax over all counted days
 *     L + 49  max_A: the largest Amax seen (a running maximum, not a sum)
 *     L + 50  n_days: days counted
 *     L + 51  n_void: days with no admissible box; they enter nothing else
 *     L + 52  n_dry: counted days with Amax1 == 0
 * then n_days_total at K W (L + 53) and n_bad, the bad pixel-hours, behind it, once per state; the state-count entry returns
 * K W (L + 53) + 2, or -2 for K, W or L out of range.  The array ACCUMULATES over any number of calls; the caller zeroes it before
 * the first.  Everything is an integer merged with integer atomics, so the state does not depend on how the days are split into
 * calls, on the workspace size or on the launch geometry.
 * depths_out: null, or [n][K][W] 64-bit integers (device, dense): Amax, -1 for a day with no admissible box; written, not added to.
 * workspace: device memory, 8-byte aligned.  The workspace-bytes entry gives the size that lets a pass take days_per_pass whole
 * days (1 .. 65535; 576 bytes per day and 120 per pixel, rounded up to 8 per day; -2 for an argument out of range); the accumulate
 * entry takes as many whole days per pass as the workspace holds, loops over the passes, and the result does not depend on it.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n, ny or nx < 1, a size above the
 * limits, a list that is empty, unsorted or out of range, a width above min(ny, nx), day_stride < 24 ny nx, a workspace too small
 * for one day) with nothing launched and no output touched.  All offsets are 64-bit. */
long rdgan_areal_state_count(int n_windows, int n_widths, int n_levels);
long rdgan_areal_workspace_bytes(long ny, long nx, long days_per_pass);
int rdgan_areal_accumulate(const float* x, long n, long day_stride, long ny, long nx, const int* windows, int n_windows,
                           const int* widths, int n_widths, const double* levels, int n_levels, long long* counts_inout,
                           long long* depths_out, void* workspace, long workspace_bytes, void* stream);

/* Scaling of hourly fields: how the variability of rain changes with the scale it is looked at -- moments and
 * histograms of box sums over dyadic boxes and aligned windows of the day.
 * hourly, n, day_stride, ny, nx and the size limits: as x for the areal entry above (ny nx <= 2^24); q(x) and the bad pixel-hours as
 * there.  space_levels = A, 0 <= A <= 6 and 2^A <= min(ny, nx).  Space level a = 0 .. A: boxes of 2^a x 2^a pixels on the dyadic grid
 * anchored at pixel (0, 0), only those wholly inside the plane (a rim narrower than 2^a is left out at level a and at no other).
 * Time level b = 0 .. 4: the aligned windows of T = 1, 2, 4, 8, 24 hours of the day.  For a day, a level pair, a box and a window, R is
 * the sum of q over the box and the window, R <= 24 * 2^33 < 2^38; a box-window that holds a bad pixel-hour is void.
 * counts_inout [(A + 1) * 5 * 296 + 2] 64-bit integers (device); the record of (a, b) lies at (a * 5 + b) * 296 +
 *     0       n_boxes: the valid box-windows
 *     1       n_void: the void box-windows
 *     2       n_wet: the valid box-windows with R > 0
 *     3       sum1: the sum of R over the valid box-windows
 *     4       sum2_hh: with R = h * 2^19 + l, l < 2^19, the sum of h^2
 *     5       sum2_hl: the sum of h l
 *     6       sum2_ll: the sum of l^2 (the second moment is 2^38 sum2_hh + 2^20 sum2_hl + sum2_ll, in integers of any width)
 *     7       max_R: the largest R seen (a running maximum, not a sum)
 *     8       hist[288]: valid box-windows by the bin of R -- bin 0: R = 0; R = 1 .. 7: bin R; otherwise, e = floor(log2 R),
 *             bin 8 + 8 (e - 3) + ((R >> (e - 3)) & 7), which covers [(8 + m) << (e - 3), (9 + m) << (e - 3)); the last is 287
 * then n_days_total at (A + 1) * 5 * 296 and n_bad, the bad pixel-hours of the planes (rims included), behind it; the state-count
 * entry returns (A + 1) * 5 * 296 + 2, or -2 for A out of range.  The array ACCUMULATES over any number of calls; the caller zeroes
 * it before the first.  Everything is an integer merged with integer atomics, so the state does not depend on how the days are split
 * into calls, on the launch geometry or on whether the array admits 16-byte loads.
 * workspace: device memory, 8-byte aligned; nothing is held in it, the workspace-bytes entry returns 8 (-2 for a shape or A out of
 * range) and the accumulate entry asks for that much.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n, ny or nx < 1, a size above the
 * limits, day_stride < 24 ny nx, A outside 0 .. 6 or 2^A > min(ny, nx), a workspace below 8 bytes) with nothing launched and no
 * output touched.  All offsets are 64-bit. */
long rdgan_scaling_state_count(int space_levels);
long rdgan_scaling_workspace_bytes(long ny, long nx, int space_levels);
int rdgan_scaling_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, int space_levels, long long* counts_inout,
                             void* workspace, long workspace_bytes, void* stream);

/* Catchment rainfall of hourly fields: the areal rainfall of every basin of a map, hour by hour, its largest
 * k-hour accumulation per day, and statistics of those maxima over the days.
 * hourly, n, day_stride, ny, nx and the size limits: as x for rdgan_areal_accumulate above (ny nx <= 2^24); q(x) and the bad
 * pixel-hours are the ones defined there.  windows and levels: as there (K <= 8, L <= 16, on the HOST).
 * The map: n_catch = C catchments, 1 <= C <= 65535.  pixels [n_entries] ints (device): the flat indices y nx + x of the pixels of
 * catchment 0, then of catchment 1, ...; a pixel may stand in several catchments or in none; C <= n_entries = E <= 2^26.
 * npix [C] ints (device): the number of pixels of each catchment, >= 1.  chunks [n_chunks][3] ints (device): (catchment, first
 * entry, count), a run of 1 <= count <= 256 consecutive entries of ONE catchment; together the chunks cover every entry once;
 * C <= n_chunks <= min(E, 2^19).  The kernels read the lists through the chunk table only, and nobody checks it on the device: the
 * caller guarantees that no chunk crosses a catchment and that every entry lies in 0 .. ny nx - 1 (a chunk that would leave the
 * lists or the state is skipped, an entry outside the plane adds nothing).
 * For day u, catchment c and hour h, P[u][c][h] is the sum of q over the catchment's pixels (a bad pixel-hour adds 0) and
 * B[u][c][h] the number of its bad pixel-hours; a catchment-hour with B > 0 is void.  For window k, A[u][c][k] is the largest
 * P[h0] + .. + P[h0 + k - 1] over the start hours h0 <= 24 - k whose k hours are all clean, h* the smallest h0 that attains it;
 * A < 2^50.  With no clean window the day is void for (c, k); with A == 0 it is dry.
 * counts_inout [C * K * (L + 30) + 2] 64-bit integers (device); the record of (c, k) lies at (c K + k) (L + 30) +
 *     0       level_count[b], b = 0 .. L: counted days by b = #{l : A >= L_q[l] npix[c]} (levels are catchment-MEAN depths)
 *     L + 1   start_hour[h], h = 0 .. 23: days with A > 0 by h*
 *     L + 25  sum_A: the sum of A over the counted days
 *     L + 26  max_A: the largest A seen (a running maximum, not a sum)
 *     L + 27  n_days: days counted (not void)
 *     L + 28  n_void: days with no clean window; they enter nothing else
 *     L + 29  n_dry: counted days with A == 0; they enter level_count, n_days and n_dry only
 * then n_days_total at C K (L + 30) and n_bad, the sum of B (a bad pixel-hour counts once per catchment that lists the pixel),
 * behind it, once per state; the state-count entry returns C K (L + 30) + 2, or -2 for C, K or L out of range.  The array
 * ACCUMULATES over any number of calls; the caller zeroes it before the first.  Everything is an integer merged with integer
 * atomics, so the state does not depend on how the days are split into calls, on the workspace size or on the launch geometry.
 * series_out: null, or [n][C][24] 64-bit integers (device, dense): P, -1 at a void catchment-hour.  depths_out: null, or [n][C][K]:
 * A, -1 for a void day.  Both written, not added to.
 * workspace: device memory, 8-byte aligned; the entry zeroes what a pass uses.  The workspace-bytes entry gives the size that lets a
 * pass take days_per_pass whole days (1 .. 65535; 288 bytes per catchment and day; -2 for an argument out of range); the accumulate
 * entry takes as many whole days per pass as the workspace holds, at most (2^24 - 1) / n_chunks, loops over the passes, and the
 * result does not depend on it.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n, ny, nx or n_catch < 1, a size above
 * the limits, a list that is empty, unsorted or out of range, day_stride < 24 ny nx, a workspace too small for one day) with
 * nothing launched and no output touched.  All offsets are 64-bit. */
long rdgan_catchment_state_count(int n_catch, int n_windows, int n_levels);
long rdgan_catchment_workspace_bytes(int n_catch, long days_per_pass);
int rdgan_catchment_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, const int* chunks, long n_chunks,
                               const int* pixels, long n_entries, const int* npix, int n_catch, const int* windows, int n_windows,
                               const double* levels, int n_levels, long long* counts_inout, long long* series_out,
                               long long* depths_out, void* workspace, long workspace_bytes, void* stream);

/* Space-time structure of hourly fields: does the rain move?  The wet/dry agreement between hour h at
 * pixel p and hour h + k at pixel p + d for every small displacement d, and for every pair of hours the displacement that best
 * maps one wet mask onto the other (the cross-correlation tracking radar nowcasting calls TREC).
 * x, n, day_stride, ny, nx, thresholds, wet and bad pixels: as for rdgan_cells_accumulate above.  W_t[i,h] is the wet mask of plane
 * (i, h) at threshold t.  radius R in 1 .. 8, max_lag K in 1 .. 6; ny, nx >= 2R + 1, ny nx <= 2^24, n 24 ny nx <= 2^40.
 * A displacement is d = (dy, dx), |dy|, |dx| <= R, dy counting rows and dx columns, with the flat index (dy + R)(2R + 1) + dx + R;
 * there are D = (2R + 1)^2 of them.  d points from the earlier hour to the later one: a positive dx means the rain moved towards
 * larger x.  Hours pair inside a day only, h = 0 .. 23 - k; days and scenarios never pair with each other.
 * Pooled counts, over every (i, h <= 23 - k), k = 0 .. K; P(d) is the set of pixels p with p and p + d both inside the plane:
 *   pairs[k][d]         p in P(d) with neither x[i,h](p) nor x[i,h+k](p + d) bad
 *   wet_first[t][k][d]  those pairs with W_t[i,h](p)
 *   wet_second[t][k][d] those pairs with W_t[i,h+k](p + d)
 *   joint[t][k][d]      those pairs with both
 * Best shift, per threshold, for k = 1 .. K and every (i, h <= 23 - k): the core C is the set of pixels with R <= y < ny - R and
 * R <= x < nx - R; A = W_t[i,h], B = W_t[i,h+k]; dist(d) = #{p in C : A(p) != B(p + d)} (a bad pixel is simply dry here).  If A
 * has no wet pixel in C or B has none in the plane, the pair is uninformative: it adds 1 to no_shift[t][k - 1] and nothing else.
 * Otherwise its shift d* minimises dist, ties going to the smaller dy^2 + dx^2, then the smaller dy, then the smaller dx; the pair
 * adds 1 to shift_hist[t][k - 1][d*], dist(d*) to dist_best[t][k - 1] and dist(0) to dist_zero[t][k - 1].
 * counts_inout [rdgan_spacetime_state_count(T, R, K)] 64-bit integers (device), flat:
 *     0                  pairs[K + 1][D]
 *     (K + 1) D + t PT   the block of threshold t, PT = (3 (K + 1) + K) D + 3 K words:
 *        + 0               wet_first[K + 1][D]
 *        + (K + 1) D       wet_second[K + 1][D]
 *        + 2 (K + 1) D     joint[K + 1][D]
 *        + 3 (K + 1) D     shift_hist[K][D]
 *        + (3 (K + 1) + K) D         no_shift[K]
 *        + (3 (K + 1) + K) D + K     dist_best[K]
 *        + (3 (K + 1) + K) D + 2 K   dist_zero[K]
 *     (K + 1) D + T PT   n_days, then n_bad_pixels, once per state
 * The array ACCUMULATES over any number of calls; the caller zeroes it before the first.  Everything is an integer merged with
 * integer atomics, so the state does not depend on how the days are split into calls, on the workspace size or on the launch
 * geometry.  The state-count entry returns -2 for T, R or K out of range.
 * workspace: device memory, 8-byte aligned; it holds the bit masks of a pass, (T + 1) ny ceil(nx / 64) 8 bytes per plane.
 * rdgan_spacetime_workspace_bytes(ny, nx, n_thresholds, planes_per_pass) is the size for planes_per_pass planes (1 .. 65520; -2
 * for an argument out of range); the entry takes as many whole DAYS per pass as the workspace holds, at least one, loops over the
 * passes, and the result does not depend on it.  16-byte loads when x is 16-byte aligned and nx and day_stride are multiples of
 * 4, a scalar path otherwise (4-byte alignment is required).  Asynchronous on the stream; 0 = success, -2 = bad argument (a null
 * or misaligned pointer, n < 1, ny or nx < 2R + 1, a size above the limits, a threshold list, radius or max_lag out of range,
 * day_stride < 24 ny nx, a workspace too small for one day) with nothing launched and no output touched.  All offsets are 64-bit. */
long rdgan_spacetime_state_count(int n_thresholds, int radius, int max_lag);
long rdgan_spacetime_workspace_bytes(long ny, long nx, int n_thresholds, long planes_per_pass);
int rdgan_spacetime_accumulate(const float* x, long n, long day_stride, long ny, long nx, const double* thresholds, int n_thresholds,
                               int radius, int max_lag, long long* counts_inout, void* workspace, long workspace_bytes, void* stream);

/* Analog baseline, the method of fragments: the k library days whose daily field most resembles a daily
 * condition, one of them picked per member, its hourly fractions scaled to the condition's daily amounts.
 * The search is defined in integers.  q(x) = (int) rintf(x * 1024).  A pixel-hour of the library is bad when x is NaN, +-inf,
 * negative or >= 2048; D[p] is the sum of q over the 24 hours (a bad hour adds 0), below 2^26; the feature is e[p] =
 * floor(sqrt(D[p])), exact, below 2^13.  A library day is VOID when it holds a bad pixel-hour or the sum of its D is 0; a void day
 * is never a neighbour.  A query is a daily sum in mm, Dq = (int) rintf(x * 1024), e = floor(sqrt(Dq)); a pixel of a query is MASKED
 * when x is NaN, +-inf, negative or >= 2048 * 24.  dist(i, j) is the sum over the unmasked pixels of query i of (e_i[p] - e_j[p])^2,
 * below 2^38, and key = dist * 2^24 + j: equal distances go to the smaller library index.  A library day whose group equals the
 * query's group, and is >= 0, is skipped.
 * Shapes: 1 <= ny nx = P <= 4096, Ppad = 8 ceil(P / 8), C = Ppad / 8; 1 <= n < 2^24 library days; 1 <= n_queries <= 2^18;
 * 1 <= k <= 32; 1 <= n_members <= 65535.  All buffers lie on the device.
 * rdgan_analog_features, hourly != 0: x [n][24][ny][nx] fp32, the leading stride day_stride >= 24 P (4-byte aligned; 16-byte loads
 * when x is 16-byte aligned and P and day_stride are multiples of 4).  feat_out: 64 ceil(n / 64) Ppad uint16, 16-byte aligned, in
 * blocks of 64 days: the 8 pixels 8c .. 8c + 7 of day j lie at byte 16 (((j / 64) C + c) 64 + j % 64); padding pixels are 0, the
 * days behind n are not written.  total_out [n] 64-bit: the sum of q over the day's pixel-hours that are not bad.  void_out [n]
 * bytes, 1 for a void day.  n_void_out [1] 64-bit: the count of void days (written, not added to).  mask_out must be null.
 * rdgan_analog_features, hourly == 0: x [n][ny][nx] fp32, day_stride == P.  feat_out and mask_out [n][Ppad] uint16, 16-byte
 * aligned: the feature, and 0xFFFF for a pixel that counts; both 0 for a masked or padding pixel.  The other outputs must be null.
 * rdgan_analog_search: lib_feat, lib_void as written above for n days of `plane` = P pixels; query_feat, query_mask likewise.
 * lib_groups [n], query_groups [n_queries] int32, null for no exclusion (both must be given to have one).  neighbours_out
 * [n_queries][k] int32 and distances_out [n_queries][k] 64-bit, by ascending key, -1 in the slots behind the admissible days;
 * found_out [n_queries] int32, the slots filled.  workspace: 8-byte aligned; rdgan_analog_workspace_bytes(n_queries, k, n_slices)
 * = n_slices n_queries 64 k bytes holds the lists of n_slices slices (-2 for an argument out of range).  The search cuts the
 * library into as many slices as the workspace holds lists for, at most one per block of 64 days, each ceil(blocks / slices)
 * blocks long; the result does not depend on it, nor on the query tile (16 queries while Ppad <= 2048, 8 above) or the geometry.
 * rdgan_analog_apply: lib [n][24][ny][nx] with day_stride, cond [n_queries][ny][nx], neighbours [n_queries][k] and found
 * [n_queries] as the search wrote them.  For query i and member m, f = found[i]: bits = rd_bits(rd_member_key(rd_make_key(seed, 9),
 * first_member + m), first_query + i) (csrc/rdgan_rng.h); weights 0 (uniform): r = (bits f) >> 32; weights 1 (1 / rank): c[r] =
 * sum over s <= r of floor(2^20 / (s + 1)), r the first index with c[r] > (bits c[f - 1]) >> 32; the donor is j = neighbours[i][r].
 * picks_out [n_queries][n_members] int32: j, -1 when f = 0.  out [n_queries][n_members][24][ny][nx] fp32: with d[p] the fp32 sum of
 * the donor's hours 0 .. 23 in that order, cond[i][p] * (lib[j][h][p] / d[p]) where d[p] > 0 and cond[i][p] * (the donor's sum
 * over the plane of hour h / its sum over the day) where d[p] = 0; NaN at a masked pixel and throughout when f = 0.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size outside the limits above, an
 * output that the mode does not write, day_stride below 24 P, a workspace too small for one slice, weights not 0 or 1, first_query
 * + n_queries above 2^32) with nothing launched and no output touched.  All offsets are 64-bit. */
long rdgan_analog_workspace_bytes(long n_queries, int k, long n_slices);
int rdgan_analog_features(const float* x, long n, long day_stride, long ny, long nx, int hourly, unsigned short* feat_out,
                          unsigned short* mask_out, long long* total_out, unsigned char* void_out, long long* n_void_out, void* stream);
int rdgan_analog_search(const unsigned short* lib_feat, const unsigned char* lib_void, const int* lib_groups, long n, long plane,
                        const unsigned short* query_feat, const unsigned short* query_mask, const int* query_groups, long n_queries,
                        int k, int* neighbours_out, long long* distances_out, int* found_out, void* workspace, long workspace_bytes,
                        void* stream);
int rdgan_analog_apply(const float* lib, long n, long day_stride, long ny, long nx, const float* cond, long n_queries,
                       long first_query, const int* neighbours, const int* found, int k, int n_members, long first_member,
                       unsigned long long seed, int weights, float* out, int* picks_out, void* stream);

/* Chaining scenarios across midnight: how well every member of one day continues every member of the next,
 * the cheapest single series through the days, and a greedy matching of the members of neighbouring days.
 * Everything is an integer.  A value x of an hourly array is GOOD when it is finite and 0 <= x < 2048; a good value has the feature
 * e = min((int) rintf(x * 32), 65535), a uint16 in units of 1/32 mm (rint to even); a bad value has the feature 0 and sets the bad
 * bit of its (day, edge, pixel).  Edge 0 of a day is its first_hour, edge 1 its last_hour, both 0 .. 23.  Boundary b joins edge 1 of
 * day b to edge 0 of day b + shift, b = 0 .. B - 1, B = n_days - shift (shift 1: a seam; shift 0: two hours of the same day).  Pixel p
 * is MASKED at boundary b when either edge's bad bit is set; n_valid[b] counts the other pixels.  C[b][i][j] is the sum over the
 * unmasked pixels of |e(day b, member i, edge 1, p) - e(day b + shift, member j, edge 0, p)|, below 2^40; a fully masked boundary
 * has all costs 0.  key = C << 24 | i << 12 | j is a strict total order of the pairs of a boundary.
 * Shapes: 1 <= ny nx = P <= 2^24, Ppad = 8 ceil(P / 8), W = ceil(Ppad / 32); 1 <= members <= 4096; 1 <= n_days <= 65535; at most
 * 2^31 costs per call.  All buffers lie on the device.
 * rdgan_seq_edges: hourly [n][24][ny][nx] fp32 with the leading stride day_stride >= 24 P (4-byte aligned; 16-byte loads when it is
 * 16-byte aligned and P and day_stride are multiples of 4); unit u is day u % n_days of member u / n_days, n a multiple of n_days.  Only the
 * two chosen hours are read.  feat_out [n][2][Ppad] uint16, 16-byte aligned, padding pixels 0.  bad_inout [n_days][2][W] 32-bit
 * words, bit p % 32 of word p / 32, ORed into: the caller zeroes it before the first call.
 * rdgan_seq_costs: feat_a [s_a][n_days][2][Ppad] and bad_a, the row ensemble; feat_b [s_b][n_days][2][Ppad] and bad_b, the column
 * ensemble (the same pointers for one ensemble).  costs_out [B][s_a][s_b] and n_valid_out [B], 64-bit (written, not added to).
 * pixel_splits: into how many ranges the pixels of a tile of pairs are cut, one workgroup each (at most one per 128 pixels); 0 leaves
 * the choice to the entry (about 2048 workgroups a launch).  The result does not depend on it, nor on how the kernel cuts the pairs
 * into tiles: integer sums, 32-bit partial sums added to 64-bit ones every 32768 pixels of a range.
 * rdgan_seq_minplus: costs [n_boundaries][S][S]; acc_out [n_boundaries + 1][S] 64-bit with acc[0] = 0 and acc[b + 1][j] = min over i
 * of acc[b][i] + C[b][i][j]; back_out [n_boundaries][S] int32, the smallest i that attains the minimum.  Costs >= 0 whose path sums
 * stay below 2^62.
 * rdgan_seq_match: costs [n_boundaries][S][S] with 0 <= C < 2^40; the greedy matching of every boundary -- all pairs walked by
 * ascending key, a pair taken when neither its row nor its column is taken -- computed as rounds of locally dominant pairs: a free
 * pair is taken iff its key is the minimum of its row over the free columns and of its column over the free rows.  init = 1 starts
 * the matchings (perm -1, free_rows S), init = 0 continues them; `rounds` rounds are launched, 0 .. 4096; a round of a complete
 * matching does nothing.  perm_inout [n_boundaries][S] int32: the column of row i, -1 while free.  free_rows_inout [n_boundaries]
 * int32.  S rounds complete any matching.  workspace: 8-byte aligned, rdgan_seq_workspace_bytes(S, n_boundaries) bytes (-2 for an
 * argument out of range), kept by the caller between the calls of one matching.  No workgroup waits for another.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size or hour outside the limits above,
 * day_stride below 24 P, n not a multiple of n_days, shift outside 0 .. n_days - 1, pixel_splits < 0, a workspace too small) with nothing launched and
 * no output touched.  All offsets are 64-bit. */
long rdgan_seq_workspace_bytes(long n_members, long n_boundaries);
int rdgan_seq_edges(const float* hourly, long n, long day_stride, long ny, long nx, long n_days, int first_hour, int last_hour,
                    unsigned short* feat_out, unsigned int* bad_inout, void* stream);
int rdgan_seq_costs(const unsigned short* feat_a, const unsigned int* bad_a, long s_a, const unsigned short* feat_b,
                    const unsigned int* bad_b, long s_b, long n_days, long plane, int shift, int pixel_splits, long long* costs_out,
                    long long* n_valid_out, void* stream);
int rdgan_seq_minplus(const long long* costs, long n_boundaries, long n_members, long long* acc_out, int* back_out, void* stream);
int rdgan_seq_match(const long long* costs, long n_boundaries, long n_members, int init, int rounds, int* perm_inout,
                    int* free_rows_inout, void* workspace, long workspace_bytes, void* stream);

/* Least-cost assignment of the members of neighbouring days: what the greedy matching above is not.
 * costs [n_boundaries][S][S] 64-bit with 0 <= C < 2^40 (not checked), the limits of the matching above: 1 <= S <= 4096,
 * 1 <= n_boundaries <= 65535, at most 2^31 costs per call.  For every boundary b: perm_out [n_boundaries][S] int32, a permutation
 * that minimises total = sum over i of C[b][i][perm[b][i]]; u_out and v_out [n_boundaries][S] 64-bit, duals with
 * u[i] + v[j] <= C[b][i][j] for all pairs and equality on the matched ones, so sum u + sum v = total proves the optimum;
 * total_out [n_boundaries] 64-bit.  Optimal permutations are not unique; the algorithm is the definition: shortest augmenting paths
 * with dual potentials (the Hungarian method in Jonker-Volgenant form), rows inserted in the order 0 .. S - 1 from u = v = 0, each by
 * a Dijkstra search over the columns whose next column is the unused one of the smallest (minv[j], j), value first, then the
 * smaller index.  |u|, |v| < S 2^40 <= 2^52: plain 64-bit integers.  One workgroup solves one boundary from the first row to the
 * last; no workgroup waits for another, every loop is counted, and the result does not depend on the launch geometry.  Outside
 * the precondition the result is not the defined one, but every access stays in range.  All buffers lie on the device.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size outside the limits) with
 * nothing launched and no output touched.  All offsets are 64-bit. */
int rdgan_assign(const long long* costs, long n_boundaries, long n_members, int* perm_out, long long* u_out, long long* v_out,
                 long long* total_out, void* stream);

/* Scenario reduction: k representative members of an ensemble of hourly days and the weight of each, by fast
 * forward selection (Heitsch & Roemisch 2003, Algorithm 2.4) under the L1 distance of integer features.
 * Everything is an integer.  A member is [n_days][24][ny][nx] fp32.  A value x is GOOD when it is finite and 0 <= x < 2048; a good
 * value has e = min((int) rintf(x * 32), 65535), in units of 1/32 mm (rint to even).  With pool = p in {1, 2, 4, 8} a feature position is
 * a p x p block of one plane, ceil(ny / p) rows of ceil(nx / p) blocks, a rim block smaller and with its own pixel count n; its feature
 * is (sum of e + n / 2) / n in integer division, a uint16, and it is BAD (feature 0) when any of its pixels is.  A member has
 * Pf = n_days 24 ceil(ny / p) ceil(nx / p) positions, padded to Ppad = 8 ceil(Pf / 8) with zeros that are never bad; W = ceil(Ppad / 32).
 * A position is MASKED when it is bad in any member; the mask is applied when distances are formed, so it does not matter in which
 * order members and bad values arrive.  Dist[i][j] = sum over the unmasked positions of |e_i - e_j|: symmetric, zero diagonal.
 * Limits: 1 <= members <= 4096, 1 <= ny nx <= 2^24, a member of at most 2^40 values, Pf 65535 members < 2^52 (so that
 * key = z << 12 | u of the selection stays inside 64 bits).  All buffers lie on the device.
 * rdgan_red_features: member m at hourly + m * member_stride, member_stride >= n_days 24 ny nx (4-byte aligned; 16-byte loads at pool 1
 * when it is 16-byte aligned and member_stride a multiple of 4).  feat_out: member m's Ppad uint16 at feat_out + m * feat_stride,
 * 16-byte aligned, feat_stride >= Ppad and a multiple of 8, padding 0.  bad_inout [W] 32-bit words, bit f % 32 of word f / 32, ORed
 * into: the caller zeroes it before the first call and passes it to every call of one ensemble.
 * rdgan_red_distances: feat as written above for all n_members, bad [W]; dist_out [n_members][n_members] and n_valid_out [1], 64-bit
 * (written, not added to): n_valid = Pf - the masked positions.  position_splits: into how many ranges the positions of a tile of
 * pairs are cut, one workgroup each (at most one per 128 positions); 0 leaves the choice to the entry (about 2048 workgroups a
 * launch).  The result does not depend on it: integer sums, 32-bit partial sums added to 64-bit ones every 32768 positions of a
 * range.  Only the tiles on and above the diagonal are computed; each sum is written to [i][j] and [j][i].
 * rdgan_red_select: dist [S][S], symmetric, 0 <= Dist < 2^52 / S (what rdgan_red_distances writes, or a distance of the caller's).
 * m[j] = +inf; step t = 0 .. k - 1, 1 <= k <= S: z[u] = sum over j of min(m[j], Dist[u][j]) for every u not yet selected, the pick is
 * the u of the smallest key = z[u] << 12 | u (ties to the smaller index), chosen_out [k] int32 = u, cost_out [k] 64-bit = z[u], then
 * m[j] = min(m[j], Dist[u][j]).  cost[t] is S times the Kantorovich distance between the ensemble and its reduction to the first
 * t + 1 picks.  assign_out [S] int32: the chosen u of the smallest Dist[u][j] << 12 | u; counts_out [k] int32: counts[t] members are
 * assigned to chosen[t], their sum is S; a pick that duplicates a smaller-indexed pick exactly gets 0.  All k steps are enqueued at
 * once.  workspace: 8-byte aligned, rdgan_red_workspace_bytes(S, k) bytes (-2 for an argument out of range).
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size, pool or k outside the limits
 * above, a stride too small or no multiple of 8, position_splits < 0, a workspace too small) with nothing launched and no output
 * touched.  All offsets are 64-bit. */
long rdgan_red_workspace_bytes(long n_members, long k);
int rdgan_red_features(const float* hourly, long n_members, long member_stride, long n_days, long ny, long nx, int pool,
                       unsigned short* feat_out, long feat_stride, unsigned int* bad_inout, void* stream);
int rdgan_red_distances(const unsigned short* feat, const unsigned int* bad, long n_members, long feat_stride, long n_positions,
                        int position_splits, long long* dist_out, long long* n_valid_out, void* stream);
int rdgan_red_select(const long long* dist, long n_members, long k, int* chosen_out, long long* cost_out, int* assign_out,
                     int* counts_out, void* workspace, long workspace_bytes, void* stream);

/* Joint-field scores of ensembles of hourly days: the energy score (Gneiting et al. 2008) and the variogram
 * score of order p (Scheuerer & Hamill 2015) of an ensemble of whole days against the observed day, taken as one vector.
 * An ensemble is x [m][24][ny][nx] fp32, every value finite, 1 <= m <= 8192; the observation y [24][ny][nx] fp32.  A position where y
 * is NaN is left out of every sum of that day; a day without a valid position has NaN in every floating-point output (and counts of
 * 0).  shared = 0: ens [n_days][m][24][ny][nx], one ensemble per day; shared = 1: ens [m][24][ny][nx], one ensemble for all days.
 * obs [n_days][24][ny][nx].  1 <= n_days <= 2^20, 1 <= ny nx <= 2^24, at most 2^40 ensemble values per call.  All buffers lie on the
 * device, dense; ens and obs 4-byte aligned, the outputs and the workspace 8-byte aligned.
 * rdgan_mv_energy: with V the valid positions of the day and |a - b| = sqrt(sum over p in V of (a_p - b_p)^2), the values converted
 * to fp64 and the differences formed and accumulated in fp64 (ascending p), obs_sum_out [n_days] = sum over i of |x_i - y| and
 * pair_sum_out [n_days] = sum over i < j of |x_i - x_j|, fp64.  Two members equal at every valid position contribute exactly 0 (the
 * difference form, not the Gram form).  The caller forms ES = obs_sum / m - pair_sum / m^2, or pair_sum / (m (m - 1)) for the fair
 * score, whose spread term is 0 at m = 1.  The sums are formed per 64 x 64 tile of the distance matrix and the tiles added in a
 * fixed order: two calls agree bit for bit and a day's sums do not depend on the other days of the call.  With shared = 1 the
 * distances among members are computed once for the days without a NaN, and once more for each day that has one.
 * rdgan_mv_variogram: p is 0.5 or 1, 0 <= radius <= 4 (pixels), 0 <= max_lag <= 3 (hours).  A displacement (l, di, dj) has 0 <= l <=
 * max_lag and |di|, |dj| <= radius and lies in the half-space l > 0, or l = 0 and di > 0, or l = 0, di = 0 and dj > 0.  A pair is
 * a = (h, i, j), b = (h + l, i + di, j + dj), both inside the day and the plane (no wrap) and both valid.  v_k = |x_k,a - x_k,b|^p in
 * fp32 (the difference rounded to fp32, sqrtf for p = 0.5), mean = (sum over k = 0 .. m - 1, in that order, of v_k in fp64) / m,
 * o = |y_a - y_b|^p likewise.  sq_out [n_days][max_lag + 1][2 radius + 1][2 radius + 1] fp64 = the sum over the pairs of
 * (o - mean)^2 at [l][di + radius][dj + radius], count_out (same shape, 64-bit integers) the number of pairs; both 0 outside the
 * half-space.  The pairs are added in a fixed order; the shared form equals the per-day form given the same ensemble n_days times,
 * bit for bit.  The caller forms VS = sum of w sq, by default w = 1 / sqrt(l^2 + di^2 + dj^2).
 * The *_workspace_bytes entries return the bytes a call with these arguments needs (-2 for an argument out of range); a larger
 * workspace changes nothing.  Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size
 * outside the limits above, shared not 0 or 1, p not 0.5 or 1, a workspace too small, more than 2^31 - 1 workgroups) with nothing
 * launched and no output touched.  All offsets are 64-bit. */
long rdgan_mv_energy_workspace_bytes(long m, long n_days, int shared);
int rdgan_mv_energy(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, double* obs_sum_out,
                    double* pair_sum_out, void* workspace, long workspace_bytes, void* stream);
long rdgan_mv_variogram_workspace_bytes(long n_days, long ny, long nx, int radius, int max_lag, int shared);
int rdgan_mv_variogram(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, double p, int radius,
                       int max_lag, double* sq_out, long long* count_out, void* workspace, long workspace_bytes, void* stream);

/* Multivariate rank histograms: the pre-ranks of the observed day among the members of an ensemble of whole
 * hourly days -- average rank and band depth (Thorarinsdottir, Scheuerer & Heinz 2016) and the leave-one-out minimum spanning tree
 * (Smith & Hansen 2004; Wilks 2004).  Everything is an integer.
 * A case is z_0 = the observation y [24][ny][nx] and z_1 .. z_m = the members x [m][24][ny][nx], fp32, N = m + 1, 1 <= m <= 4095.  A
 * position is VALID when all N values are finite there (a NaN or an infinity of the observation or of any member leaves it out).
 * Per valid position and per i, comparing in fp32 (-0.0 == 0.0): lt_i = the number of j with z_j < z_i, gt_i those with z_j > z_i.
 * shared = 0: ens [n_days][m][24][ny][nx]; shared = 1: ens [m][24][ny][nx], one ensemble for all days.  obs [n_days][24][ny][nx].
 * 1 <= n_days <= 2^20, 1 <= ny nx <= 2^24, N 24 ny nx <= 2^40 and at most 2^40 ensemble values per call.  All buffers lie on the
 * device, dense; ens and obs 4-byte aligned, the outputs and the workspace 8-byte aligned.
 * rdgan_mvr_ranks: sums_out [n_days][24][N][2], 64-bit, index 0 of N the observation: per hour h, [i][0] = the sum over the hour's
 * valid positions of lt_i - gt_i + N + 1 (twice the mid-rank of z_i, so ties need no randomness) and [i][1] = the sum of
 * (N - 1)(N - 2) - lt_i (lt_i - 1) - gt_i (gt_i - 1) (twice the number of pairs of the other vectors whose closed interval holds
 * z_i: the band depth; low is outlying).  n_valid_out [n_days][24], 64-bit: the hour's valid positions.  Both are written, not added
 * to; the caller adds the hours for the day.  A position whose N values are all equal adds N + 1 and (N - 1)(N - 2) to every i in
 * closed form; the result is the same with and without that shortcut.  position_runs: into how many runs the tiles of positions
 * of a plane are cut, one workgroup each; 0 leaves the choice to the entry (about 2048 workgroups a launch).  The result does not
 * depend on it: integer sums met by 64-bit integer atomics.  workspace: 8-byte aligned, rdgan_mvr_ranks_workspace_bytes(m, n_days,
 * shared) bytes (-2 for an argument out of range); nothing is kept in it today.
 * rdgan_mvr_mst: dist [n][n] 64-bit, symmetric, 0 <= entries < 2^40 (what rdgan_red_distances writes for Pf 65535 < 2^40; the
 * caller checks), 1 <= n <= 4096.  len_out [n], 64-bit: len[i] = the length of the minimum spanning tree of the n - 1 vertices other
 * than i (Prim's algorithm, one workgroup per i); 0 for n <= 2.  The weights are integers, so the length does not depend on the
 * order in which equal edges are taken.  Outside the precondition the result is not the defined one, but every access stays in
 * range.
 * Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size outside the limits above, shared
 * not 0 or 1, position_runs < 0, a workspace too small, more than 2^31 - 1 workgroups) with nothing launched and no output touched.
 * All offsets are 64-bit. */
long rdgan_mvr_ranks_workspace_bytes(long m, long n_days, int shared);
int rdgan_mvr_ranks(const float* ens, const float* obs, long m, long n_days, long ny, long nx, int shared, int position_runs,
                    long long* sums_out, long long* n_valid_out, void* workspace, long workspace_bytes, void* stream);
int rdgan_mvr_mst(const long long* dist, long n, long long* len_out, void* stream);

/* Random-cascade baseline: the microcanonical multiplicative cascade (Olsson 1998; Guentner et al. 2001) with
 * the three-way first split of a 24-hour day (Mueller & Haberlandt 2015).  rdgan_cascade_accumulate counts, over observed hourly
 * data, how a wet box of rain splits into its parts; the caller turns the counts into a table of thresholds; rdgan_cascade_generate
 * applies the splits recursively to daily sums: 24 h -> 3 x 8 h -> 4 h -> 2 h -> 1 h.  Everything is an integer.
 * Units: q(x) = (int) rintf(x * 1024).  A pixel-hour is bad when x is NaN, +-inf, negative or >= 2048.  A pixel-day with a bad hour is
 * left out whole and counted in n_bad; one with sum 0 is counted in n_dry and adds nothing else.
 * Tree: node 0 is the day, split into thirds of 8 h; nodes 1 .. 3 the 8 h boxes (level 0), 4 .. 9 the 4 h boxes (level 1), 10 .. 21
 * the 2 h boxes (level 2), each split into halves.  A node of volume V = 0 is not a sample.  edge_units [n_edges], host memory: the
 * edges of the volume classes as integers per hour, rint(mm/h * 1024), strictly increasing in 1 .. 2^21, 0 <= n_edges <= 7 (null for
 * none); the class of a box of `hours` hours is the number of edges e with V >= e * hours, NV = n_edges + 1.  Position class of a box
 * of a binary level, from whether the previous and the next box of its level within the day are wet (beyond the day's ends: dry):
 * 0 isolated, 1 starting (previous dry, next wet), 2 enclosed, 3 ending.  Type of a binary split with first half V1: 0 = 0/1 (V1 = 0),
 * 1 = 1/0 (V1 = V), 2 = x/(1-x) with the weight bin b = (V1 * 32) / V.  The day: its pattern is the wet mask of the thirds (bit t:
 * third t); two wet thirds: the bin of the first wet one, (V_first * 32) / V; three: b1 = (V1 * 32) / V and b2 = (V2 * 32) / (V - V1).
 * State, rdgan_cascade_state_size(n_edges) = 748 NV + 3 64-bit counters (-2 for n_edges out of range), flat in this order:
 *     0          type    [level 3][position 4][NV][3]
 *     36 NV      weight  [level 3][position 4][NV][32]
 *     420 NV     pattern [NV][8]
 *     428 NV     w2      [NV][pattern 8][32]          (patterns 3, 5, 6)
 *     684 NV     w3a     [NV][32]                     b1 of pattern 7
 *     716 NV     w3b     [NV][32]                     b2 of pattern 7
 *     748 NV     n_days, n_bad, n_dry                 pixel-days seen, left out for a bad hour, without rain
 * rdgan_cascade_accumulate: hourly [n][24][ny][nx] fp32 on the device, the leading stride day_stride >= 24 ny nx (4-byte aligned; 16-byte
 * loads when it is 16-byte aligned and ny nx and day_stride are multiples of 4), ny nx <= 2^24, at most 2^40 elements.  state_inout
 * (device, 8-byte aligned) ACCUMULATES over any number of calls; the caller zeroes it before the first.  Integer atomics throughout:
 * the state does not depend on how the days are split into calls or on the launch geometry.
 * rdgan_cascade_generate: model [748 NV] uint32 on the device, the state's layout without the last three words: per row the
 * cumulative thresholds c[j] = (cum[j] << 24) / total, non-decreasing, the last 2^24 (and c[0] = 0 in a pattern row); a draw r < 2^24
 * picks the first j with c[j] > r.  cond [n_queries][ny][nx] fp32 daily sums in mm; a pixel is masked when it is NaN, +-inf, negative
 * or >= 16384 and gets 24 NaNs (units -1); otherwise V = rint(cond * 1024) < 2^24 is split level by level, the position classes of a
 * level taken from the wetness the level above produced, and the children of a node sum to its V exactly.
 * Draws: key = rd_member_key(rd_member_key(rd_make_key(seed, 10), first_member + m), first_query + i) for member m of query i, r =
 * rd_bits(key, (block * 32 + node) * 4 + draw) >> 8 (csrc/rdgan_rng.h), block = (y / patch) ceil(nx / patch) + x / patch: the pixels
 * of a patch x patch block share their draws.  Draw 0 picks the type or the pattern, draw 1 the bin b, draw 2 the 24 bits u inside
 * it: part(V, b, u, most) = min(max((V ((b << 24) + u)) >> 29, 1), most), a 64-bit product.  The day: while the pattern has more wet
 * thirds than V has units, its highest wet third is dropped; two wet thirds: the first gets part(V, b, u, V - 1), b from w2; three:
 * V1 = part(V, b1, u1, V - 2) with b1 from w3a, then of R = V - V1, V2 = part(R, b2, u2, R - 1) with b2 from w3b and the draws 1 and
 * 2 of node 22.  A binary node of V >= 2: the type from its row; type 2 gives V1 = part(V, b, u, V - 1).  A binary node of V = 1 cannot
 * split x/(1-x): with (c0, c1, 2^24) its row, type 0 where (r c1) >> 24 < c0 and type 1 otherwise; where c1 = 0, type 0 for r < 2^23.
 * out [n_queries][n_members][24][ny][nx] fp32 = units * 2^-10, exact; a pixel's 24 hours sum to rint(cond * 1024) / 1024.  units_out:
 * null, or int32 of the same shape.  16-byte stores when nx is a multiple of 4 and out and units_out are 16-byte aligned.
 * 1 <= n_queries <= 2^18, 1 <= n_members <= 65535, at most 2^40 output values, 1 <= patch <= 2^24, first_query + n_queries <= 2^32,
 * 0 <= first_member <= 2^62.  Asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, a size, an
 * edge list, patch, first_query or first_member outside the limits above, day_stride below 24 ny nx) with nothing launched and no
 * output touched.  All offsets are 64-bit. */
long rdgan_cascade_state_size(int n_edges);
int rdgan_cascade_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, const int* edge_units, int n_edges,
                             long long* state_inout, void* stream);
int rdgan_cascade_generate(const unsigned* model, const int* edge_units, int n_edges, const float* cond, long n_queries,
                           long first_query, long ny, long nx, int n_members, long first_member, unsigned long long seed, int patch,
                           float* out, int* units_out, void* stream);

/* Extremes of hourly fields (csrc/rdgan_extremes.hip.h): block maxima of the k-hour depths of every pixel, and
 * the integer sums that give the L-moments of series of such maxima.
 * The block-maxima entry: hourly, n, day_stride, ny, nx and the size limits as x for rdgan_areal_accumulate (ny nx <= 2^24); q(x) and a
 * bad pixel-hour as there.  A pixel-day with a bad hour is void.  block [n] ints on the HOST: the block of every day, each in
 * 0 .. n_blocks - 1 = NB - 1, in any order (1 <= NB <= 2^31).  window_mask: bit w - 1 set for a window of w hours, 1 .. 8 bits
 * among the low 24, K their number; window i is the i-th set bit from below.  The depth of a good pixel-day for window w is the
 * largest q[h0] + .. + q[h0 + w - 1] over h0 = 0 .. 24 - w: windows lie within the day and never cross midnight.
 *   bmax_inout [NB][K][ny nx] 64-bit integers (device): the largest depth of any good day of the block; the caller fills it with -1
 *     before the first call, and -1 stays where a block has no good day.  NB K ny nx <= 2^31.
 *   ndays_inout, nvoid_inout [NB][ny nx] 32-bit integers (device): the good and the void pixel-days; zeroed by the caller.
 * The three ACCUMULATE over any number of calls through integer atomics (max and add), so they do not depend on how the days are
 * split into calls, on their order or on days_per_run: the days a workgroup walks before it hands over, 1 .. 4096, or 0 for the
 * entry's choice.
 * rdgan_lmoment_sums: table [S][B][M] 64-bit integers (device), S = n_series series of B = n_blocks maxima (1 <= B <= 128) at
 * M = n_positions positions, S B M <= 2^40.  An entry below 0 is left out; with ndays ([S][B][M] 32-bit integers, device, or null)
 * so is one whose ndays entry is below min_days.  The entries kept must be below 2^40 (the caller checks).  Over their ascending
 * order statistics x_(1) <= .. <= x_(n):
 *   sums_out [S][M][3]: A0 = sum x_(j), A1 = sum (j - 1) x_(j), A2 = sum (j - 1)(j - 2) x_(j), each below 2^40 128^3 = 2^61
 *   n_out [S][M] 32-bit integers: n
 *   sorted_out: null, or [S][B][M]: x_(1) .. x_(n), then -1 for every entry left out
 * Written, not added to; invariant under the order of tied values and independent of the launch geometry.
 * Both asynchronous on the stream; 0 = success, -2 = bad argument (a null or misaligned pointer, n, ny, nx, S, B or M < 1, a size
 * above the limits, B > 128, a window mask that is 0 or has more than 8 bits or one above bit 23, a block outside 0 .. NB - 1,
 * day_stride < 24 ny nx, days_per_run outside 0 .. 4096) with nothing launched and no output touched.  All offsets are 64-bit. */
int rdgan_block_maxima_accumulate(const float* hourly, long n, long day_stride, long ny, long nx, const int* block, long n_blocks,
                                  unsigned window_mask, int days_per_run, long long* bmax_inout, int* ndays_inout, int* nvoid_inout,
                                  void* stream);
int rdgan_lmoment_sums(const long long* table, const int* ndays, int min_days, long n_series, int n_blocks, long n_positions,
                       long long* sums_out, int* n_out, long long* sorted_out, void* stream);

/* Log-spectral distance, log_spectral_distance.py.  rdgan_spectra_bins: K, the radial bins kept for an nd x nd field
 * (nd 8/16/24/32/48/64: 3/9/15/20/32/43); -2 for an nd the spectra kernel does not cover.
 * rdgan_radial_spectra: compute_radial_spectrum (:59-65) with azimuthal_average (:19-56) -- fields [n][nd][nd] fp32 ->
 * out [n][K] = mean of |fftshift(fft2(x))|^2 over the integer radial bins 1..K about the centre ((nd-1)/2, (nd-1)/2) (bin 0,
 * which holds DC, and the corner bin are dropped, as the reference's bookkeeping drops them); log_out != 0 writes
 * 10 log10 of it (dB; -inf for an empty bin).  An all-zero or constant field gives 0 (-inf dB) in every kept bin. */
int rdgan_spectra_bins(int nd);
int rdgan_radial_spectra(const float* fields, float* out, long n, int nd, int log_out, void* stream);
/* rdgan_lsd_pairwise: log_spectral_distance (:68-77) for every ordered pair of compute_dists (:104-118), reduced on the device.
 * spec_a [n][k], spec_b [m][k] are log-spectra in dB (spec_b may equal spec_a); d(i, j) = sqrt(sum (a_i - b_j)^2) * (1/k) in
 * fp32, NaN for two empty spectra and +inf for one (log10(0/0), log10(p/0) of the reference).  Outputs, NULL to skip, not
 * all NULL: dist [n][m] fp32; hist [nbins + 4] uint64 = counts per bin b = (int)floorf((d - lo) * scale), scale = (float)nbins
 * / (hi - lo), all fp32, clamped to nbins - 1, then d < lo, d >= hi, NaN, +inf; moments [5] = count, sum, sum of squares
 * (fp64), min, max of the finite d, which needs workspace of rdgan_lsd_workspace_bytes(n, m).  exclude_diagonal != 0
 * leaves the pairs i == j out of hist and moments and writes 0 there in dist (:112 never writes them, :123-130 removes them).
 * hist and moments are the same bit for bit on every call.  n, m <= 2^22; 1024 k + 4 (nbins + 4) <= 57344 with hist
 * (512 bins at any k; 2048 at k <= 47); k <= 48. */
long rdgan_lsd_workspace_bytes(long n, long m);
int rdgan_lsd_pairwise(const float* spec_a, const float* spec_b, long n, long m, int k, int exclude_diagonal, float* dist,
                       unsigned long long* hist, int nbins, float lo, float hi, double* moments, void* workspace,
                       long workspace_bytes, void* stream);

/* RainFARM baseline, rainfarm/rainfarm_temporal_downscaling.py (R below); nd 8/16/24/32/48/64, 24 hours; -2 for any other nd.
 * rdgan_rainfarm_classes: C = (nd/2 + 1)^2 + 13, the length of the class arrays of rdgan_rainfarm_slope_stats.
 * rdgan_rainfarm_slope_stats: the statistics behind estimate_alpha (R:54-81) and estimate_beta (R:22-51), in fp64 arithmetic, for
 * samples [n][24][nd][nd] fp32 (16-byte aligned): per frequency class, the number of kept points (counts, uint64) and the sum of
 * log(|F|^2) over them (sums, fp64).  Classes 0 .. (nd/2+1)^2 - 1: the 2-D DFT of every hour plane, class |a| (nd/2 + 1) + |b| for
 * the integer fftfreq indices (a, b) of the point; then 13 classes |m| = 0 .. 12 of the 24-point DFT of every pixel series.  A point
 * is kept when its power is > 0 and its frequency is not 0.  Repeated calls agree bit for bit.  n <= 2^24; workspace of
 * rdgan_rainfarm_stats_workspace_bytes(n, nd).  The fit (_log_slope, R:6-19) runs on the host over the classes. */
int rdgan_rainfarm_classes(int nd);
long rdgan_rainfarm_stats_workspace_bytes(long n, int nd);
int rdgan_rainfarm_slope_stats(const float* samples, long n, int nd, unsigned long long* counts, double* sums, void* workspace,
                               long workspace_bytes, void* stream);
/* rdgan_rainfarm_generate: downscale_spatiotemporal (R:84-125) for n members in fp32.  amplitudes [24][nd][nd] complex (re, im fp32
 * pairs) = R's sqrt(om^-beta k^-alpha) with its zeroing (R:103-113, built on the host); precip [nd][nd] for every member
 * (precip_per_member = 0) or [n][nd][nd]; phases u from uniforms [n][24][nd][nd] (fp32, or fp64 when uniforms_fp64; R:103's
 * np.random.rand) or, when uniforms is NULL, from the counter RNG: u = rd_uniform(rd_member_key(rd_make_key(seed,
 * RD_STREAM_RAINFARM), first_member + i), e) for member i and element e = (t nd + y) nd + x (rdgan_rng.h).
 * out [n][24][nd][nd] = r precip / sum_t r, r = exp(g / std(g)), g = Re ifftn(amplitudes e^{2 pi i u}) (R:114-122); exact 0 where
 * precip is 0.  n <= 2^24; workspace of rdgan_rainfarm_gen_workspace_bytes(n). */
long rdgan_rainfarm_gen_workspace_bytes(long n);
int rdgan_rainfarm_generate(const float* amplitudes, const float* precip, int precip_per_member, const void* uniforms,
                            int uniforms_fp64, uint64_t seed, long first_member, float* out, long n, int nd,
                            void* workspace, long workspace_bytes, void* stream);

/* Op-level entry points used by the parity tests (tests/test_hip_ops.py). */
/* Conv3D forward, TF semantics.  x [B,D,H,W,Cin] -> y [B,Do,Ho,Wo,Cout]; upsample=1 folds
 * UpSampling3D(2) in front (T:330-331); pad = zero padding before each axis; Cin%4==0,
 * Cout%64==0 (or 32). */
int rdgan_op_conv3d(const float* x, const float* w, const float* bias, float* y, int B, int D, int H,
                    int W, int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d,
                    int pad_h, int pad_w, int upsample, void* stream);
/* the same contraction with bf16 operands (x and w rounded to nearest-even bf16 on the device, fp32 accumulation;
 * v_mfma_f32_32x32x16_bf16): the GEMM of the "bf16" storage mode.  out_bf16 = 0: y is fp32 (the arithmetic, checked at
 * 1e-5 against the oracle on bf16-rounded operands); 1: y is bf16 (2 bytes per element), the accumulator rounded once
 * after the epilogue, as the storage mode writes it; 2: as 1 through k_conv_gemm_f16 ("conv_f16"; Cout % 128 == 0, else -2).
 * No folded upsample; Cin, Cout % 64 == 0. */
int rdgan_op_conv3d_bf16(const float* x, const float* w, const float* bias, float* y, int B, int D, int H,
                         int W, int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d,
                         int pad_h, int pad_w, int out_bf16, void* stream);
/* input gradient of the above for stride 2 (parity-phase plan) or stride 1: gy -> gx (same dims as x,
 * on the upsampled grid when the forward had upsample=1: D,H,W are the conv's input extents). */
int rdgan_op_conv3d_dgrad(const float* gy, const float* w, float* gx, int B, int D, int H, int W,
                          int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h,
                          int pad_w, void* stream);
/* the same input gradient with bf16 operands (gy, w rounded to bf16; fp32 accumulation): Cin, Cout % 64 == 0. */
int rdgan_op_conv3d_dgrad_bf16(const float* gy, const float* w, float* gx, int B, int D, int H, int W,
                               int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h,
                               int pad_w, void* stream);
/* weight gradient dW [3,3,3,Cin,Cout] of the forward above. */
int rdgan_op_conv3d_wgrad(const float* x, const float* gy, float* dw, int B, int D, int H, int W,
                          int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h,
                          int pad_w, int upsample, void* stream);
/* weight gradient with bf16 operands (x, gy rounded to bf16; fp32 accumulation and output): Cin % 128 == 0 and
 * Cout % 64 == 0, or Cin == 64 and Cout % 128 == 0 (tiles of 128 or 256 rows). */
int rdgan_op_conv3d_wgrad_bf16(const float* x, const float* gy, float* dw, int B, int D, int H, int W,
                               int Cin, int Cout, int Do, int Ho, int Wo, int stride, int pad_d, int pad_h,
                               int pad_w, void* stream);
/* Weight gradient of one tap group (g = 0, 1, 2) of the shared-centre form of a generator block through the production
 * plan (4 parity phases x 4 taps: the even tap count that selects the 256-row tile at B*D*H*W >= 65536).  g = 0: src = E
 * [B,D+1,H,W,Cin], dy [B,2D,2H,2W,Cout] (even planes used); g = 1: src = x [B,D,H,W,Cin], dy = plane-pair sums
 * [B,D,2H,2W,Cout]; g = 2: E at j = s+1 against the odd planes.  dU [48][Cin][Cout], forms g*16 .. g*16+15 written.
 * bf16 = 1: operands rounded to bf16 on the device, fp32 accumulation (Cin % 128 == 0). */
int rdgan_op_fastd_wgrad(const float* src, const float* dy, float* dU, int B, int D, int H, int W, int Cin, int Cout,
                         int g, int bf16, void* stream);
/* Weight gradient of the last generator conv (64 -> 1; backward of T:345) alone, through the production kernels:
 * dW[27][64] from dl [B][24][nd][nd] and h3 [B][24][nd][nd][64].  kernel = 1: the matrix-pipe kernel (k_g9_wgrad_mfma),
 * 0: the scalar kernel it replaced (k_g9_wgrad_pairs; nd <= 72); bf16 = 1: h3 rounded to bf16 first (storage mode). */
int rdgan_op_g9_wgrad(const float* dl, const float* h3, float* dW, int B, int nd, int bf16, int kernel, void* stream);
/* Generator block 3 forward of the bf16 storage mode (T:340-343 on the 12 x 8 x 8 x 128 input of ndomain 16) through the slab
 * kernel alone (k_upconv_slab16): x and w are rounded to bf16 on the device, y = LeakyReLU(PixelNorm(upconv(x) + bias)) comes
 * back as fp32 (the bf16 output widened), rinv [B,24,16,16] = 1/l2 per grid point; dbg: NULL, or [B*24*16*16][4] floats (test
 * hook: row sum of squares and 1/l2 as the two lane halves of a row computed them). */
int rdgan_op_upconv_slab16(const float* x, const float* w, const float* bias, float* y, float* rinv, float* dbg, int B, void* stream);
/* The same block of the large-domain variant (L:355-358; source planes of H x W positions, multiples of 8: 32 x 32 at ndomain 64)
 * through the tiled slab kernel alone (k_upconv_slab_t16: 8 x 8 tiles with their halo resident, K in two halves):
 * x [B,12,H,W,128], y [B,24,2H,2W,64], rinv [B,24,2H,2W], dbg NULL or [B*24*2H*2W][4]. */
int rdgan_op_upconv_slab_t16(const float* x, const float* w, const float* bias, float* y, float* rinv, float* dbg, int B, int H, int W,
                             void* stream);
/* Generator block 2 forward of the bf16 storage mode (T:335-338 on the 6 x 4 x 4 x 256 input of ndomain 16) through the slab kernel
 * alone (k_upconv2_slab16): x and w [3,3,3,256,128] are rounded to bf16 on the device, y [B,12,8,8,128] = LeakyReLU(PixelNorm(
 * upconv(x) + bias)) comes back as fp32 (the bf16 output widened), rinv [B,12,8,8] = 1/l2 per grid point. */
int rdgan_op_upconv2_slab16(const float* x, const float* w, const float* bias, float* y, float* rinv, int B, void* stream);
/* Weight gradient of generator block 3 in the collapsed form (backward of T:340-341 on the 12 x 8 x 8 x 128 input of ndomain 16)
 * through the slab kernel of the bf16 storage mode alone (k_upconv_wgrad_slab16): x [B,12,8,8,128] and dy [B,24,16,16,64] (gradient
 * at the conv output) are rounded to bf16 on the device; dWc [64 = phase*8 + tap][128][64] fp32 -- entry (phase, tap) is the sum over
 * samples and source positions r of x[r + off(phase, tap)] (outer) dy[2 r + phase], off = phase - 1 + tap per axis. */
int rdgan_op_upconv_wgrad_slab16(const float* x, const float* dy, float* dWc, int B, void* stream);
/* Forward of the critic's second layer (T:291-293, Conv3D(128, 3x3x3, stride 2, 'same') on 11 x 7 x 7 x 64 + bias + LeakyReLU +
 * dropout) through the slab kernel of the bf16 storage mode alone (k_d2_fwd_slab16): x [B,11,7,7,64] and w [3,3,3,64,128] are rounded
 * to bf16 on the device, y [B,6,4,4,128] comes back as fp32 (the bf16 output widened); seed = 0: dropout off. */
int rdgan_op_d2_fwd_slab16(const float* x, const float* w, const float* bias, float* y, int B, uint64_t seed, void* stream);
/* Weight gradient of the critic's second layer (backward of T:291, Conv3D(128, 3x3x3, stride 2, 'same') on 11 x 7 x 7 x 64) through
 * the slab kernel of the bf16 storage mode alone (k_d2_wgrad_slab16): x [B,11,7,7,64] (layer 1's output) and dy [B,6,4,4,128] are
 * rounded to bf16 on the device; dW [3,3,3,64,128] fp32 = sum over samples and output positions o of x[2 o + tap - 1] (outer) dy[o]. */
int rdgan_op_d2_wgrad_slab16(const float* x, const float* dy, float* dW, int B, void* stream);
/* the same through the tiled kernel of the larger domains (k_d2_wgrad_slab_t16: work items = 4 x 4 tiles of output positions with the
 * layer-1 positions their taps reach, one halo position per odd class): x [B,11,2 OH - 1,2 OW - 1,64], dy [B,6,OH,OW,128], OH and OW
 * multiples of 4 (ndomain 32 / 48 / 64: OH = ndomain / 4). */
int rdgan_op_d2_wgrad_slab_t16(const float* x, const float* dy, float* dW, int B, int OH, int OW, void* stream);
/* Weight gradient of the critic's third layer (backward of T:295, Conv3D(256, 3x3x3, stride 2, 'same') on 6 x 4 x 4 x 128 ->
 * 3 x 2 x 2 x 256) through the slab kernel of the bf16 storage mode alone (k_d3_wgrad_slab16): x [B,6,4,4,128] (layer 2's output) and
 * dy [B,3,2,2,256] are rounded to bf16 on the device; dW [3,3,3,128,256] fp32 = sum over samples and o of x[2 o + tap] (outer) dy[o]. */
int rdgan_op_d3_wgrad_slab16(const float* x, const float* dy, float* dW, int B, void* stream);
/* Input gradient of the critic's second layer (backward of T:291, Conv3D(128, 3x3x3, stride 2, 'same') on the 11 x 7 x 7 x 64
 * output of layer 1, ndomain 16) through the slab kernel of the bf16 storage mode alone (k_d2_dgrad_slab16): gy [B,6,4,4,128], the
 * layer's kernel w [3,3,3,64,128] and aux [B,11,7,7,64] (layer 1's output) are rounded to bf16 on the device;
 * gx [B,11,7,7,64] = conv3d_input_grad(gy, w) * gate(aux), as fp32; gate = LeakyReLU'(aux), and with use_drop != 0 aux is read as
 * a stored post-dropout activation: +0.0 = dropped (gate 0), anything else kept (gate LeakyReLU'(aux) / 0.75). */
int rdgan_op_d2_dgrad_slab16(const float* gy, const float* w, const float* aux, float* gx, int B, int use_drop, void* stream);
/* The same through the tiled kernel of the larger domains (k_d2_dgrad_slab_t16; L:291-293): gy [B,6,OH,OW,128], aux and gx
 * [B,11,2 OH - 1,2 OW - 1,64]; OH, OW multiples of 4 (ndomain 32 / 48 / 64: 8 / 12 / 16). */
int rdgan_op_d2_dgrad_slab_t16(const float* gy, const float* w, const float* aux, float* gx, int B, int OH, int OW, int use_drop,
                               void* stream);
/* PixelNormalization + LeakyReLU(0.2) forward (T:255-266, T:333) and its backward. C in {64,128,256}. */
int rdgan_op_pixelnorm_lrelu(const float* y, float* h, float* rinv, long npix, int C, void* stream);
int rdgan_op_pixelnorm_lrelu_bwd(const float* gh, const float* h, const float* rinv, float* dy,
                                 long npix, int C, void* stream);
/* ---- The step's elementwise kernels one by one (test hooks).  Each launches the production kernel through the launcher the
 * step functions use (csrc/rdgan_elem_launch.h): same grid, same split.  Raw device pointers, fp32 unless said otherwise; -2 on a
 * bad argument. ----
 * Tail of the last generator conv (T:345-350): the remaining tap sums + bias, Softmax over the 24 hours, check_numerics.
 * out [B,24,H,W]; *flag is OR-ed with 1 when a logit or an output is NaN/Inf, and never cleared.  (The reference checks the softmax
 * output only; a lone -Inf logit gives p = 0 there and passes.  Flagging it is stricter; finite inputs are unaffected.)  taps by form:
 *   0  k_colgather_softmax: P[B*24*H*W][32], column t = (kd*3+kh)*3+kw holds h3[pos] . W9[t]; logit(pos) = bias + sum_t P[pos+t-1][t]
 *   3  k_tapsum_softmax<24,3>: Q[b][d][3][h][w], entry kd = the sum over (kh,kw) of the products plane d sends to plane d+1-kd
 *      at (h,w); logit(d) = bias + sum_kd Q[d+kd-1][kd]
 *   9  k_tapsum_softmax<24,9>: Q[b][d][9][h][w], entry (kd,kh) = the sum over kw sent to (d+1-kd, h+1-kh, w);
 *      logit(d,h) = bias + sum_{kd,kh} Q[d+kd-1][kd*3+kh][h+kh-1]
 *   12 k_tapsum_softmax12 (H = W = 16): QT[b][item 0..5][tp 0..5][p 0..3][q 0..3][64]; item = planes 4 item .. 4 item + 3, tp = target
 *      plane 4 item - 1 + tp, p = source parity class, q = target class 2 (y&1) + (x&1) at class position (y>>1)*8 + (x>>1);
 *      logit(d,y,x) = bias + sum over the items that reach plane d, and over p, of QT[..][q(y,x)][pos(y,x)]
 * (The tiled variant k_tapsum_softmax12t with k_g9_halo_fold has no entry: the fused-last-conv test ties it to the separate pass.) */
int rdgan_op_softmax_tail(int form, const float* taps, const float* bias, float* out, int* flag, int B, int H, int W, void* stream);
/* Softmax backward (k_softmax_bwd): dl = p * (g - sum_d p g) per (sample, h, w) column; p, g, dl [B,24,H,W]. */
int rdgan_op_softmax_bwd(const float* p, const float* g, float* dl, int B, int H, int W, void* stream);
/* Gradient-penalty norm (T:238-241; k_gp_norm_part + k_gp_norm_r0): g0 [B][per]; gp_out [B] = ||g0[b]|| - 1; cin_hat_out [B][per][CP],
 * channel 0 = (10/B) 2 (n-1)/n g0, channels 1..CP-1 = 0.  force_S = 0: the step's choice of workgroups per sample, else that many
 * (1..64).  A sample of norm 0 gets gp = -1 and NaN in its cin_hat rows (0 * inf, as the gradient of Keras's sqrt). */
int rdgan_op_gp_norm(const float* g0, int B, int per, int CP, int force_S, float* cin_hat_out, float* gp_out, void* stream);
/* Loss tails.  mode 0 (k_critic_losses, T:215-216, T:388-392): v [2B] = critic values real | fake, gp [B]; out8 = (total, mean(-v_real),
 * mean(v_fake), mean(gp^2), flag, 0, 0, 0), total = the second + the third + 10 x the fourth.  mode 1 (k_gen_loss, T:408): v [B];
 * out8 = (mean(-v), 0, 0, 0, flag, 0, 0, 0).  flag = 1 when the total is NaN/Inf or gflag_in != 0 (the generator's check_numerics). */
int rdgan_op_loss_tail(int mode, const float* v, const float* gp, int B, int gflag_in, float* out8, void* stream);
/* The critic's Dense layer (T:303-304; k_critic_dense_fwd) and the top of its input-gradient chain (k_critic_top_bwd) over NB samples
 * of F features: v_out [NB] = h4 . w + bias; u4_out [NB][F] = gate(h4) w dv(sample), dv = -1/B | +1/B | 1 for the thirds of the 3B
 * batch (mode 0) or -1/B (mode 1); gate = LeakyReLU' of the stored output (1 where h4 > 0, else 0.2), and with seed != 0 additionally
 * 0 where h4 is +0.0 (dropped) and 1/0.75 elsewhere.  bf16 != 0: h4 and u4_out are bf16 buffers. */
int rdgan_op_critic_dense(const void* h4, const float* w, const float* bias, float* v_out, void* u4_out, int NB, int F, int B, int mode,
                          uint64_t seed, int bf16, void* stream);
/* Dense weight gradient (k_critic_dense_wgrad + the fold of its row slices): out [F] = sum_b buf[b][:] dv(b) over NB = 3B samples;
 * slices = 0: the step's choice, else that many row slices (16 at the most).  bf16 != 0: buf is a bf16 buffer. */
int rdgan_op_critic_dense_wgrad(const void* buf, float* out, int NB, int F, int B, int slices, int bf16, void* stream);
/* Weight forms of a generator block's kernel W [27][CC] (CC = Cin Cout, CC % 4 == 0) and their adjoints.  which = 0
 * (k_collapse_weights / k_fold_collapsed_wgrad): out [64 = phase(pd,ph,pw) * 8 + tap(ad,ah,aw)][CC], per axis the sum of the taps
 * p = 0: {0} | {1,2}, p = 1: {0,1} | {2}.  which = 1 (k_weight_transform / k_weight_transform_adj): out [48 = g * 16 + (ph * 2 + th)
 * * 4 + (pw * 2 + tw)][CC], along d the groups g = 0: -W0, 1: W0 + W1 + W2, 2: W2, on h and w the collapsed sums.  _adj: dforms
 * [64 | 48][CC] -> dW [27][CC] = the transposed map. */
int rdgan_op_weight_forms(int which, const float* W, float* out, long CC, void* stream);
int rdgan_op_weight_forms_adj(int which, const float* dforms, float* dW, long CC, void* stream);
/* Critic input (T:275-282, T:221-224; k_build_critic_input[_v4]): real, fake [B][D][HW], cond [B][HW][nc]; out [B | 3B][D][HW][CP]
 * = (sample | the nc condition channels | zeros).  mode 0: real | fake | alpha real + (1 - alpha) fake with alpha[b] = the uniform
 * of key (seed, stream 5) at counter alpha_base + b; mode 1: fake only; mode 2: real only.  scalar != 0 forces the one-voxel kernel
 * where the step would take the four-voxel one (nc = 1, CP = 2, HW % 4 == 0). */
int rdgan_op_critic_input(const float* real, const float* fake, const float* cond, float* out, int B, int D, int HW, int nc, int CP,
                          int mode, uint64_t seed, uint32_t alpha_base, int scalar, void* stream);
/* Gradient wrt the generator's Dense pre-activation (T:326-328).  k_pool_lrelu_bwd: out [B,D,H,W,C] = (sum of the 8 children of
 * gup [B,2D,2H,2W,C]) * LeakyReLU'(h0); k_lrelu_bwd: out [n] = g * LeakyReLU'(h), n % 4 == 0, bf16 != 0: g and h are bf16 buffers. */
int rdgan_op_pool_lrelu_bwd(const float* gup, const float* h0, float* out, int B, int D, int H, int W, int C, void* stream);
int rdgan_op_lrelu_bwd(const void* g, const void* h, float* out, long n, int bf16, void* stream);
/* Column sums behind every bias gradient (k_colsum_partial / k_colsum_partial_any + the fold), through the handle's partial buffer:
 * out [C] = sum over rows of src [rows][C].  bf16 != 0 (C in {64, 128, 256}): src is a bf16 buffer. */
int rdgan_op_colsum(rdgan_handle* h, const void* src, long rows, int C, float* out, int bf16, void* stream);
/* Hour differences of the shared-centre form and their adjoint (k_diff_d, k_combine_dx), P floats per hour plane (P % 4 == 0):
 * x [B][D][P] -> E_out [B][D+1][P] = x[j] - x[j-1] (x zero outside); dx_inout [B][D][P] += dE[d] - dE[d+1], dE [B][D+1][P].  Either
 * pair may be NULL.  bf16 != 0: all four are bf16 buffers. */
int rdgan_op_diff_combine(const void* x, void* E_out, void* dx_inout, const void* dE, int B, int D, long P, int bf16, void* stream);
/* Test hook: copies the first n floats of an activation tensor the last forward pass left in the workspace into `out`
 * (device, fp32): which = 0..3 generator h0..h3 [B, D, H, W, C] after LeakyReLU; 4..7 critic layers 1..4 after LeakyReLU
 * and dropout ([B] samples after a generator step or a critic forward; [3B] = real | fake | interpolated after a critic step,
 * whose interpolated third is only meaningful with the option "keep_gates": without it the second sweep of the gradient penalty
 * has overwritten it).  The gradient parity tests take the LeakyReLU slope pattern of the run from here, so that the fp64
 * oracle differentiates the same piecewise-linear branch.  which = 8 (bf16 storage mode, ndomain 16, option "d2_gate_bits"): the packed
 * gate bytes of critic layer 1 as floats, 16 per row: byte q of a row = channels 4 q .. 4 q + 3, two bits each (bit 0: output > 0,
 * bit 1: dropped). */
int rdgan_debug_activation(rdgan_handle* h, int which, float* out, long n, void* stream);
/* Test hook (fp32 storage): the first critic layer's input gradient with respect to the sample channel, g0_out [B][24][nd][nd],
 * from a given output gradient u1 [B][L1][64] (device, fp32) by the route the steps take (option "d1_dgrad_fused").  with_norm != 0:
 * as the critic step's gradient-penalty sweep, also gp_out [B] = ||g0|| - 1 and cin_hat_out [B][24 nd nd][CP] = the second sweep's
 * input (r0, 0).  Asynchronous on `stream`; overwrites the critic workspace. */
int rdgan_debug_d1_input_grad(rdgan_handle* h, const float* critic_params, const float* u1, int B, int with_norm,
                              float* g0_out, float* cin_hat_out, float* gp_out, void* stream);
/* dropout keep-scale mask (0 or 1/0.75) and uniforms of the counter RNG, for pinning it to oracle/rng.py */
int rdgan_op_rng(uint64_t seed, uint32_t stream_id, float* mask_out, float* uniform_out, long n,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif
