/*
 * srpde.h -- C ABI of libsrpde_hip.so, the MI355X (gfx950) kernels behind the
 * superresolution_for_pdes_amd drop-in for tahmidawal/Superresolution_for_PDEs.
 *
 * The reference is pure Python (no FFI layer); its hot path dispatches PyTorch aten ops
 * from src/models.py and SciPy's SuperLU from src/data_generation.py.  Each entry point
 * below replaces the aten / SciPy call(s) cited next to it.  The Python binding is
 * superresolution_for_pdes_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a
 * maintainer would add on the reference side.
 *
 * Conventions
 *  - All tensor arguments are caller-owned DEVICE pointers; the library never allocates,
 *    frees or synchronises the host (one exception: srpde_poisson_cg_batched for a single problem
 *    too large for one cooperative grid, n > 1024).  Scratch is passed in as (workspace, ws_bytes), its
 *    size queried with the matching *_workspace_size() function.
 *  - Activations are NHWC fp32 ("channels-last").  A view is (pointer, ld): ld = floats
 *    between consecutive pixels, so channel slices of a wider tensor (virtual concat) need
 *    no copy.  Channel counts and ld must be multiples of 4; pointers 16-byte aligned.
 *  - Every call is stream-ordered on `stream` (on ROCm torch.cuda.current_stream().cuda_stream).
 *  - The library holds no global mutable state and reads no environment: every choice (kernel family,
 *    test hooks) is an argument of the call, so calls are re-entrant from any thread.  (The one piece of
 *    per-thread state is diagnostic: srpde_last_error / srpde_last_kernel.)
 *  - Return: 0 on success, negative on a bad argument (-1 arg, -2 shape, -3 alignment,
 *    -4 workspace too small), positive hipError_t on a launch failure.  srpde_last_error()
 *    returns the thread-local message of the last failure.
 */
#ifndef SRPDE_H_
#define SRPDE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

/* ABI version: bumped whenever an exported signature or a documented buffer layout changes.
 * A binding built against this header checks srpde_version() == SRPDE_ABI_VERSION at load time
 *  and refuses a mismatched library instead of misreading arguments.
 *   1  round 1-2 layout
 *   4  round 3 changes (srpde_conv_fwd_h3: in_scale ... ep_amax before the workspace; the
 *      srpde_prepare_weights_h3 descriptor row grew to 10 columns; srpde_conv_wgrad_h3p reads dy
 *      planes with a row stride of cout rounded up to 32) and round 4's additions
 *      (srpde_conv_h4_set, srpde_poisson_debug_abort)
 *   5  srpde_conv_fwd_h3: x1_ca, x1_sa before the workspace
 *   6  srpde_conv_fwd: ep_mean, ep_invstd, ep_gamma, ep_beta, ep_amax before the workspace
 *   7  srpde_conv_fwd_h3: x0_up, up_ld, up_h, up_w before the workspace; srpde_upsample_gate_sa;
 *      srpde_conv_head_eval
 *   8  srpde_conv_h3_stats_rows_for, srpde_conv_h5_set (the h5 forward writes 80-row statistics),
 *      srpde_conv_head_eval_supported, srpde_last_kernel
 *   9  srpde_conv_wgrad_h3x, srpde_conv_wgrad_h3x_supported, srpde_bn_train_finalize_ws,
 *      srpde_bn_finalize_workspace_size
 *  10  no global state: srpde_conv_h5_set / _h4_set / _h3r_set and srpde_poisson_debug_abort removed; the kernel
 *      family is SRPDE_FAM_* bits of srpde_conv_fwd_h3's / _presplit's accumulate argument and of
 *      srpde_conv_h3_stats_rows_for's new flags argument, the grid-CG abort hook a negative rtol;
 *      srpde_conv_wgrad_h3g_supported, srpde_att_pool_bn_bwd(_blocks); srpde_att_bwd takes dx == NULL
 *  11  srpde_upsample_bilinear_bwd_gated_bn, srpde_upsample_bwd_bn_supported, srpde_gating_bn_reduce(_blocks),
 *      srpde_att_bwd_params_lowres, srpde_conv_wgrad_bnb
 *  12  the batched cascade: srpde_cascade_level_stats(_workspace_size), srpde_cascade_level_assemble,
 *      srpde_cascade_stitch_denorm, srpde_field_metrics(_workspace_size)
 *  13  the direct sine-transform Poisson solver: srpde_poisson_dst_plan(_size), srpde_poisson_dst_lds_max_n,
 *      srpde_poisson_dst_workspace_size, srpde_poisson_dst_batched, srpde_poisson_dst_apply
 *  14  the device-side sample stream: srpde_stream_raw, srpde_stream_draw, srpde_stream_window
 *  15  the PDE residual as a loss term and a metric: srpde_physics_loss_workspace_size, srpde_physics_loss_fwd,
 *      srpde_physics_loss_bwd, srpde_pde_residual_metrics(_workspace_size)
 *  16  overlapping-tile cascade levels without ground truth: srpde_tiled_tiles_per_side,
 *      srpde_tiled_level_stats(_workspace_size), srpde_tiled_assemble, srpde_tiled_blend_denorm
 *  17  weighted-Jacobi sweeps of the discrete equation, blocked in LDS: srpde_pde_relax_sweeps_per_launch,
 *      srpde_pde_relax_workspace_size, srpde_pde_relax
 *  18  the divergence-form operator div(theta grad u) and its sine-preconditioned CG: srpde_div_apply,
 *      srpde_div_cg_workspace_size, srpde_div_cg_done_offset, srpde_div_cg_init, srpde_div_cg_iterate,
 *      srpde_div_cg_finish
 *  19  the divergence-form operator in the smoother and the physics loss: srpde_div_relax_workspace_size,
 *      srpde_div_relax, srpde_physics_loss_div_workspace_size, srpde_physics_loss_div_fwd
 *  20  the adjoint of the divergence-form operator and a warm-started CG: srpde_div_theta_grad,
 *      srpde_div_cg_init_from
 *  21  the shifted operator D_theta - sigma I and implicit time steps: srpde_div_apply_shift,
 *      srpde_poisson_dst_shift_batched, srpde_div_cg_init_shift, srpde_div_cg_init_from_shift,
 *      srpde_div_cg_iterate_shift, srpde_div_step_rhs
 *  22  zero-flux (Neumann) sides for the divergence-form operator and its CG: srpde_div_apply_bc,
 *      srpde_div_step_rhs_bc, srpde_div_theta_grad_bc, srpde_div_cg_workspace_size_bc, srpde_div_cg_init_bc,
 *      srpde_div_cg_init_from_bc, srpde_div_cg_iterate_bc, srpde_poisson_sep_plan(_size),
 *      srpde_poisson_sep_workspace_size, srpde_poisson_sep_shift_batched
 *  23  zero-flux sides in the smoother and the physics loss: srpde_div_relax_bc, srpde_physics_loss_div_fwd_bc
 *      extended, the number kept (entries were added, none changed: a binding built against the earlier 23 header
 *      reads every argument as before): boundary values and prescribed fluxes for the divergence-form operator,
 *      srpde_div_apply_bd, srpde_div_step_rhs_bd, srpde_div_cg_init_from_bd, srpde_div_theta_grad_bd,
 *      srpde_div_bd_grad, srpde_div_relax_bd
 *      extended again, in the same way: the face fluxes of the divergence-form operator and their wall totals,
 *      srpde_div_face_flux, srpde_div_face_flux_grad, srpde_div_wall_flux, srpde_div_wall_flux_grad
 *      extended again, in the same way: boundary data in the physics loss and the sample stream,
 *      srpde_physics_loss_div_fwd_bd, srpde_stream_walls */
#define SRPDE_ABI_VERSION 23

/* Kernel-family bits (per call; bit 0 of the same argument is the accumulate flag): the forward / dgrad
 * families compute the same outputs, statistics and stored splits bit for bit, so these only route a call to
 * another kernel -- tests compare the families, tuning times them.  SRPDE_FAM_NO_H5: not the W = 40 h5 kernel
 * (nor out_conv2's 16-output kernel); SRPDE_FAM_NO_H4: not the h4 one-tap-ring kernel (W = 10 / 20 / 40 tiles);
 * SRPDE_FAM_NO_H3R: not the 4-wave, two-workgroups-per-CU kernel for <= 64-channel tiles. */
#define SRPDE_FAM_NO_H5 2
#define SRPDE_FAM_NO_H4 4
#define SRPDE_FAM_NO_H3R 8

const char* srpde_last_error(void);
/* Name of the main kernel the last conv entry point (srpde_conv_fwd*, srpde_conv_dgrad_h3_bnb, srpde_conv_wgrad*,
 * srpde_conv_head_eval) launched on this thread, as profilers print it, e.g. "conv_fwd_h5_kernel<2, 8>" (template
 * arguments included, namespace and parameter list dropped).  Diagnostics / per-kernel roofline accounting. */
const char* srpde_last_kernel(void);
int srpde_version(void);

/* ---- convolution: nn.Conv2d 3x3 (dilation 1|2) / 1x1 -------------------------------
 * replaces aten::convolution (fwd) and aten::convolution_backward (dgrad, wgrad) for
 * ConvBlock.conv1/conv2 (src/models.py:16,18,22-23), bridge[0]/[3] (models.py:43,46),
 * out_conv1/out_conv2 (models.py:57,59).  torch.cat (models.py:87,90,93) is absorbed as
 * the (x1, c1) second input.  stats (nullable): per row-block (mean, M2) float2
 * partials for the train-mode BatchNorm that follows; srpde_conv_stats_blocks() blocks
 * of srpde_conv_stats_rows_per_block() rows each. */
int srpde_pack_conv_weights(const float* w, float* wfwd, float* wdgrad, int cout, int cin, int cin_real,
                            int ksize, hipStream_t stream);
int srpde_conv_fwd(const float* x0, int c0, int ldx0, const float* x1, int c1, int ldx1, const float* wpack,
                   const float* bias, float* y, int ldy, int n, int h, int w, int cout, int ksize, int dil,
                   int sign, int accumulate, float* stats, const float* ep_mean, const float* ep_invstd,
                   const float* ep_gamma, const float* ep_beta, unsigned* ep_amax, void* workspace,
                   size_t ws_bytes, hipStream_t stream);
/* ep_* (nullable, eval mode, layers with cin % 32 != 0 -- enc1.conv1): the epilogue applies the
 * following BatchNorm (running statistics) + ReLU, as srpde_conv_fwd_h3's ep_* below. */
/* optional scratch for splitting the last, partially filled round of tiles over K (pass
 * NULL to disable); srpde_conv_fwd_workspace_size() bytes always suffice */
size_t srpde_conv_fwd_workspace_size(int cout);
size_t srpde_conv_stats_blocks(int n, int h, int w, int cout);
int srpde_conv_stats_rows_per_block(int cout);
size_t srpde_conv_wgrad_workspace_size(int n, int h, int w, int cout, int cin, int ksize);
int srpde_conv_wgrad(const float* dy, int lddy, const float* x0, int c0, int ldx0, const float* x1, int c1,
                     int ldx1, float* dw, int cin_real, int accumulate, int n, int h, int w, int cout, int ksize,
                     int dil, void* workspace, size_t ws_bytes, hipStream_t stream);
/* srpde_conv_wgrad (fp32 kernels, one input) whose dY is the BN (+ReLU, flags SRPDE_BN_RELU) backward of the
 * layer's BatchNorm, applied as the operand is loaded: dy = gamma invstd (dz - m1 - xhat m2), dz = da masked by
 * the BN output > 0, y the BN input -- srpde_bn_relu_bwd's dy bit for bit from srpde_bn_bwd_prepare's m1 / m2,
 * never written (enc1.conv1, models.py:16-23 with the input image: no dgrad reads dy). */
int srpde_conv_wgrad_bnb(const float* da, int ldda, const float* y, int ldy, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const float* m1, const float* m2, int flags,
                         const float* x0, int c0, int ldx0, float* dw, int cin_real, int accumulate, int n, int h,
                         int w, int cout, int ksize, int dil, void* workspace, size_t ws_bytes, hipStream_t stream);
/* h3: the same convolution (forward / dgrad, same output and statistics layout) from
 * two-piece fp16 splits with power-of-two operand scales: three partial products per fp32
 * product on v_mfma_f32_32x32x16_f16, halo-staged activation tiles (conv_h3.hip).
 * amax0/amax1: device words holding max|x0| / max|x1| as float bits (any upper bound within a
 * few orders of magnitude works; srpde_absmax or the amax output of srpde_bn_relu_fwd/_bwd).
 * wsplit/wexp: srpde_split_weights_h3 of the packed weights ([2][rows][K] fp16, [rows] int).
 * xsplit_out (nullable): receives the scaled hi / lo fp16 pieces of the input, [2][P][c0+c1],
 * for srpde_conv_wgrad_h3p (the split is computed anyway; storing it costs one 4-B write per
 * element). */
int srpde_conv_h3_supported(int c0, int c1, int cout, int w, int dil, int ksize);
/* Rows per BatchNorm-statistics block written by srpde_conv_fwd_h3 (stats / bn_part buffers
 * hold ceil(P / rows) blocks); the other conv families use srpde_conv_stats_rows_per_block. */
int srpde_conv_h3_stats_rows(void);
/* Rows per BatchNorm-statistics block srpde_conv_fwd_h3 writes for the FORWARD of this shape (input
 * channels c0 + c1 -> cout at h x w, dilation dil) and kernel-family bits `flags` (those the forward call
 * will pass): 80 where the h5 kernel takes it (w = 40, h % 8 == 0, cout 64 or 32, c0 + c1 a multiple of 64,
 * no SRPDE_FAM_NO_H5), else srpde_conv_h3_stats_rows().  Dgrad partials (bn_part) keep
 * srpde_conv_h3_stats_rows(). */
int srpde_conv_h3_stats_rows_for(int c0, int c1, int cout, int h, int w, int dil, int flags);
int srpde_split_weights_h3(const float* w, void* planes, int* wexp, int rows, int K, hipStream_t stream);
int srpde_absmax(const float* x, int ldx, int c, long long P, unsigned* amax, hipStream_t stream);
/* every conv layer's forward and dgrad h3 planes in one launch from torch's [Cout][Cin][3][3]
 * weights: desc = device int64 [nlayers][10] = {w, cout, cin_real, cin_pad, planes_f, exp_f,
 * planes_d, exp_d, first row, cout_pad}; a layer owns cout forward rows then cin_pad dgrad rows of
 * K = 9 * cout_pad (k = tap * cout_pad + n, zero for n >= cout) */
int srpde_prepare_weights_h3(const long long* desc, int nlayers, int total_rows, hipStream_t stream);
/* dgrad (conv^T) with the BatchNorm (+ReLU) backward apply of the layer fused into the operand
 * transform: dy = gamma*invstd*(dz - m1 - xhat*m2) is formed per halo element from da (the BN
 * output gradient) and bn_y_in (the BN input), never stored in fp32; m1, m2 and the dy scale bound
 * from srpde_bn_bwd_prepare.  dysplit_out [2][P][cout_dy] fp16: dy's split for
 * srpde_conv_wgrad_h3p.  bn_* / bn_part (nullable): the next BN's backward reduction as in
 * srpde_conv_fwd_h3; dx_max (nullable): per output tile max|dx| (ceil(P/256)*ceil(cin_dx/BN)
 * slots) for the next srpde_bn_bwd_prepare.  Replaces srpde_bn_relu_bwd + srpde_conv_fwd_h3(sign -1). */
int srpde_conv_h3_bnb_supported(int cout_dy, int cin_dx, int w, int dil);
int srpde_conv_dgrad_h3_bnb(const float* da, int ldda, const unsigned* dy_amax, const float* bn_y_in, int bn_ldy_in,
                            const float* mean, const float* invstd, const float* gamma, const float* beta,
                            const float* m1, const float* m2, int flags, const void* wsplit, const int* wexp,
                            float* dx, int lddx, int n, int h, int w, int cout_dy, int cin_dx, int dil,
                            void* dysplit_out, const float* bn_y, int bn_ldy, const float* bn_mean,
                            const float* bn_invstd, const float* bn_gamma, const float* bn_beta, void* bn_part,
                            float* dx_max, void* workspace, size_t ws_bytes, hipStream_t stream);
/* srpde_conv_fwd_h3 (no virtual concat, no input transform) on an input that arrives as its h3
 * split: xsplit = [2][P][c] fp16 hi / lo planes of x * 2^h3_exp(*amax) (srpde_bn_bwd_apply_split,
 * or a stored xsplit_out).  The halo tiles go into the MFMA operand layout as fp16 pieces (no fp32
 * tile, no split work, nothing stored for the weight gradient, which reads the same planes); same
 * outputs, statistics, bn_part and out_max as srpde_conv_fwd_h3 on that split. */
int srpde_conv_fwd_h3_presplit(const void* xsplit, int c, const unsigned* amax, const void* wsplit, const int* wexp,
                               const float* bias, float* y, int ldy, int n, int h, int w, int cout, int ksize,
                               int dil, int sign, int accumulate, float* stats, const float* bn_y, int bn_ldy,
                               const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                               const float* bn_beta, void* bn_part, float* out_max, void* workspace, size_t ws_bytes,
                               hipStream_t stream);
/* Output tiles (= out_max slots) of srpde_conv_fwd_h3 for P rows, cin -> cout; 0 if unsupported. */
long long srpde_conv_h3_tiles(long long P, int cin, int cout, int w, int dil);
int srpde_conv_fwd_h3(const float* x0, int c0, int ldx0, const float* x1, int c1, int ldx1, const unsigned* amax0,
                      const unsigned* amax1, const void* wsplit, const int* wexp, const float* bias, float* y, int ldy,
                      int n, int h, int w, int cout, int ksize, int dil, int sign, int accumulate, float* stats,
                      void* xsplit_out, const float* in_scale, const float* in_shift, const float* bn_y,
                      int bn_ldy, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                      const float* bn_beta, void* bn_part, float* out_max, const float* ep_mean,
                      const float* ep_invstd, const float* ep_gamma, const float* ep_beta, unsigned* ep_amax,
                      const float* x1_ca, const float* x1_sa, const float* x0_up, int up_ld, int up_h, int up_w,
                      void* workspace, size_t ws_bytes, hipStream_t stream);
/* accumulate: bit 0 = y += conv; the SRPDE_FAM_* bits route the call away from a kernel family (tests /
 * tuning: the families' outputs are equal bit for bit); srpde_conv_fwd_h3_presplit reads it the same way. */
/* x1_ca [n][c1] / x1_sa [P] (nullable, together, c1 > 0): the second input is an AttentionGate's
 * input x (models.py:119-130) and the conv reads its gated output (x * ca[sample][c]) * sa[pixel]
 * (srpde_att_apply_fwd's expression, formed in the operand transform; xsplit_out and the statistics
 * are those of the gated input) -- the gated tensor is never written.
 * x0_up (nullable; up_ld its row stride, up_h = h / 2, up_w = w / 2): x0 is the bilinear x2
 * (align_corners) upsample of this [n][up_h][up_w][c0] tensor, formed in the operand transform from
 * its low-res rows (models.py:70, 89, 92: the decoder's upsampled input is never written); bit-identical
 * to reading srpde_upsample_bilinear_fwd's output.  Forward only, no in_scale, and the h4 shapes
 * (W 20 with 128-column tiles, W 40 with 64); x0 / ldx0 are ignored for the x0 channels; amax0 must
 * bound |up(x0_up)| (the source's max word does: interpolation is a convex combination).
 * ep_mean / ep_invstd / ep_gamma / ep_beta (nullable, eval mode; no stats / bn_part / accumulate):
 * the epilogue applies the following BatchNorm with its running statistics and the ReLU,
 * y = relu((conv + bias - mean) * invstd * gamma + beta) (srpde_bn_eval_prepare's mean / invstd),
 * so the conv output is the activation itself (models.py:22-23 in eval mode); ep_amax (nullable,
 * zeroed beforehand) receives max|y|, the next h3 consumer's operand-scale word.
 * out_max (nullable): every output tile writes max|y| of its elements to out_max[tile]
 * (ceil(P/rows) x ceil(cout/cols) slots, the h3 tile of the call) -- the scale bound that
 * srpde_bn_bwd_prepare needs when y is the gradient of a BN output.
 * in_scale / in_shift (nullable, c1 == 0 only): the input is relu(x0 * in_scale[c] + in_shift[c])
 * -- the producing BatchNorm + ReLU applied on the fly (srpde_bn_affine); padding stays zero.
 * bn_part (nullable; dgrad of a conv whose input was a BN + ReLU output, accumulate == 0): the
 * output is that activation's gradient, and the epilogue also writes the BN backward's
 * reduction, (sum dz, sum dz*xhat) per (srpde_conv_stats_rows_per_block(cout)-row block,
 * channel) into bn_part [srpde_conv_stats_blocks][cout] float2 (bn_y = the BN's input, its batch
 * mean / invstd, gamma / beta) -- for srpde_bn_relu_bwd_part */
/* weight gradient with the h3 arithmetic (same workspace as srpde_conv_wgrad; c0, c1, cout % 32 == 0);
 * amax_dy / amax0 / amax1: the max|.| words of dy, x0, x1 as for srpde_conv_fwd_h3 */
int srpde_conv_wgrad_h3(const float* dy, int lddy, const unsigned* amax_dy, const float* x0, int c0, int ldx0,
                        const unsigned* amax0, const float* x1, int c1, int ldx1, const unsigned* amax1, float* dw,
                        int cin_real, int accumulate, int n, int h, int w, int cout, int ksize, int dil,
                        void* workspace, size_t ws_bytes, hipStream_t stream);
/* h3 weight gradient from pre-split operands: dyp = the xsplit_out of the dgrad call (sign -1,
 * [2][P][cout]) or srpde_bn_bwd_apply_split's planes ([2][P][cout rounded up to 32]: cout = 16 reads
 * 32-channel planes), and xp = the xsplit_out of the forward call ([2][P][c0+c1]), with the max|.|
 * words those calls used.  No split work inside; workspace: srpde_conv_wgrad_h3p_workspace_size. */
size_t srpde_conv_wgrad_h3p_workspace_size(int n, int h, int w, int cout, int cin, int ksize);
int srpde_conv_wgrad_h3p(const void* dyp, const unsigned* amax_dy, const void* xp, int c0, const unsigned* amax0,
                         int c1, const unsigned* amax1, float* dw, int cin_real, int accumulate, int n, int h, int w,
                         int cout, int ksize, int dil, void* workspace, size_t ws_bytes, hipStream_t stream);
/* 1 when srpde_conv_wgrad_h3p runs this shape on the input-row-ring kernel for 128-channel m tiles
 * (conv_wgrad_h3g_kernel: cout 128, cin 32 .. 128 in steps of 32, w = 20, dilation 1 -- enc2.conv1 / conv2 and
 * dec2.conv2, models.py:80-81, 92); else the h3p / h3h tiles. */
int srpde_conv_wgrad_h3g_supported(int cout, int cin, int w, int dil);
/* srpde_conv_wgrad_h3p for the 40 x 40 layers (cout <= 64, c0 and c1 multiples of 32: shapes for which
 * srpde_conv_wgrad_h3x_supported returns 1) with the input read from its fp32 rows instead of a stored split,
 * so the forward need not write xsplit_out: in_scale / in_shift and x1_ca / x1_sa (nullable, in pairs) repeat
 * the forward call's input transform and amax0 / amax1 are that call's words -- the operand is bit for bit
 * the split the forward would have stored, and dw equals srpde_conv_wgrad_h3p's on it.  Workspace:
 * srpde_conv_wgrad_h3p_workspace_size. */
int srpde_conv_wgrad_h3x_supported(int c0, int c1, int cout, int w, int dil);
int srpde_conv_wgrad_h3x(const void* dyp, const unsigned* amax_dy, const float* x0, int ldx0, int c0,
                         const unsigned* amax0, const float* in_scale, const float* in_shift, const float* x1, int ldx1,
                         int c1, const unsigned* amax1, const float* x1_ca, const float* x1_sa, float* dw, int cin_real,
                         int accumulate, int n, int h, int w, int cout, int ksize, int dil, void* workspace,
                         size_t ws_bytes, hipStream_t stream);

/* ---- BatchNorm2d + ReLU -------------------------------------------------------------
 * replaces aten::native_batch_norm / native_batch_norm_backward and relu /
 * threshold_backward for every nn.BatchNorm2d (src/models.py:17,19,44,47,58,60) and the
 * F.relu / nn.ReLU after it (models.py:22-23,45,48,96-97). */
int srpde_bn_train_finalize(const float* stats, int nblk, int rows_per_blk, long long P, int C,
                            float* running_mean, float* running_var, long long* num_batches_tracked,
                            float momentum, float eps, float* mean_out, float* invstd_out, hipStream_t stream);
/* srpde_bn_train_finalize followed by srpde_bn_affine of its mean / invstd, in one launch (the same
 * outputs, bit for bit; amax_bound nullable, zeroed beforehand). */
int srpde_bn_train_finalize_affine(const float* stats, int nblk, int rows_per_blk, long long P, int C,
                                   float* running_mean, float* running_var, long long* num_batches_tracked,
                                   float momentum, float eps, float* mean_out, float* invstd_out, const float* gamma,
                                   const float* beta, float* scale, float* shift, unsigned* amax_bound,
                                   hipStream_t stream);
/* Either of the two above in two coalesced passes through a workspace of srpde_bn_finalize_workspace_size(nblk, C)
 * bytes (row slices of 16-channel groups, then one thread per channel over the slices): a 40 x 40 layer's
 * 20,480 partials per channel take a few microseconds instead of ~36.  gamma / beta / scale / shift /
 * amax_bound nullable (scale and shift together: the _affine outputs).  The fp64 sums run per slice, then over
 * the slices, so mean / invstd can differ from srpde_bn_train_finalize's in the last bit of the fp64 sums. */
size_t srpde_bn_finalize_workspace_size(int nblk, int C);
int srpde_bn_train_finalize_ws(const float* stats, int nblk, int rows_per_blk, long long P, int C, float* running_mean,
                               float* running_var, long long* num_batches_tracked, float momentum, float eps,
                               float* mean_out, float* invstd_out, const float* gamma, const float* beta, float* scale,
                               float* shift, unsigned* amax_bound, void* workspace, size_t ws_bytes,
                               hipStream_t stream);
int srpde_bn_eval_prepare(const float* running_mean, const float* running_var, int C, float eps, float* mean_out,
                          float* invstd_out, hipStream_t stream);
/* amax (nullable): *amax = max(*amax, max|out|) as float bits -- the operand-scale word of the
 * h3 convolutions; the caller zeroes it before the producing call */
int srpde_bn_relu_fwd(const float* y, int ldy, const float* mean, const float* invstd, const float* gamma,
                      const float* beta, float* out, int ldo, long long P, int C, int relu, unsigned* amax,
                      hipStream_t stream);
/* srpde_bn_relu_fwd of an [n][h][w][C] block output followed by srpde_maxpool2x2_fwd of it
 * (models.py:22-23 then :79-80), in one pass: out = relu(bn(y)) and pool = its 2x2 max (same
 * values and tie order as the separate calls).  h, w even. */
int srpde_bn_relu_pool_fwd(const float* y, int ldy, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, float* out, int ldo, float* pool, int ldp, int n, int h, int w, int C,
                           int relu, unsigned* amax, hipStream_t stream);
/* srpde_bn_relu_pool_fwd (ReLU always) with one block per sample, which also forms the channel branch
 * of the AttentionGate reading the activation (models.py:106-112, 119-121; as srpde_att_channel_fwd:
 * m [n][C], hbuf [n][C/8], ca [n][C]).  C a multiple of 32, <= 256.  pool == NULL: no pooling (the
 * activation and the channel branch only).  out == NULL: the activation is not written (y already is
 * it: pass mean 0, invstd 1, gamma 1, beta 0, an exact identity on y >= 0). */
int srpde_bn_relu_pool_att_fwd(const float* y, int ldy, const float* mean, const float* invstd, const float* gamma,
                               const float* beta, float* out, int ldo, float* pool, int ldp, int n, int h, int w,
                               int C, unsigned* amax, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* m, float* hbuf, float* ca, hipStream_t stream);
/* srpde_bn_relu_fwd (ReLU) that also forms the spatial attention of the gate whose gating input the
 * result is (models.py:124-125): sa[p] = sigmoid(sum_c wg[c] out[p][c] + bg[0]).  C 256, 512 or 1024.
 * out == NULL: the activation is not written (as srpde_bn_relu_pool_att_fwd). */
int srpde_bn_relu_gate_fwd(const float* y, int ldy, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, float* out, int ldo, long long P, int C, const float* wg,
                           const float* bg, float* sa, unsigned* amax, hipStream_t stream);
/* train-mode BN folded into a per-channel affine for a consumer that applies it on the fly
 * (a = relu(y*scale + shift), srpde_conv_fwd_h3's in_scale / in_shift), plus a rigorous bound
 * on max|a| (|gamma| sqrt(P-1) + |beta|, Samuelson's inequality) into *amax_bound (nullable) */
int srpde_bn_affine(const float* mean, const float* invstd, const float* gamma, const float* beta, int C, long long P,
                    float* scale, float* shift, unsigned* amax_bound, hipStream_t stream);
size_t srpde_bn_relu_bwd_workspace_size(long long P, int C);
/* backward flags (the `relu` argument of the two calls below):
 *   SRPDE_BN_RELU  the BN output went through ReLU (mask dz by the recomputed output > 0)
 *   SRPDE_BN_EVAL  the forward normalised with the running statistics (eval mode): mean / invstd
 *                  are constants, dy = gamma*invstd*dz without the batch-statistic terms
 *                  (aten native_batch_norm_backward with training=False) */
#define SRPDE_BN_RELU 1
#define SRPDE_BN_EVAL 2
/* srpde_bn_relu_bwd with the (sum dz, sum dz*xhat) reduction already done by the producer of da
 * (srpde_conv_fwd_h3's bn_part, nblk row blocks): skips the reduction pass over y and da */
int srpde_bn_relu_bwd_part(const float* y, int ldy, const float* da, int ldda, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, float* dy, int lddy, float* dgamma, float* dbeta,
                           float* dbias, long long P, int C, int relu, unsigned* amax, const void* part, int nblk,
                           void* workspace, size_t ws_bytes, hipStream_t stream);
/* The BN backward prepared for a consumer that applies it on the fly (srpde_conv_dgrad_h3_bnb):
 * dgamma, dbeta, dbias, the float vectors m1 = sum(dz)/P and m2 = sum(dz*xhat)/P, and a rigorous
 * bound on max|dy| (float bits) for the consumer's operand scale.  part (nullable): the
 * (sum dz, sum dz*xhat) partials of the dgrad that produced da, with that dgrad's per-tile
 * max|da| slots (da_max[n_da_max]); null: a reduction pass over y and da here. */
size_t srpde_bn_bwd_prepare_workspace_size(long long P, int C);
int srpde_bn_bwd_prepare(const float* y, int ldy, const float* da, int ldda, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, long long P, int C, int flags, const void* part,
                         int nblk_part, const float* da_max, int n_da_max, float* m1, float* m2, float* dgamma,
                         float* dbeta, float* dbias, unsigned* dy_amax, void* workspace, size_t ws_bytes,
                         hipStream_t stream);
/* The BN (+ReLU) backward apply with srpde_bn_bwd_prepare's m1 / m2 (the expressions of
 * srpde_bn_relu_bwd) written as the h3 operand split of dy: planes = [2][P][Cp] fp16 hi / lo of
 * dy * 2^h3_exp(*dy_amax) (dy_amax = prepare's bound), Cp = C rounded up to a multiple of 32 with
 * channels C..Cp-1 zero (out_bn2's C = 16), the input of srpde_conv_fwd_h3_presplit (c = Cp) and
 * srpde_conv_wgrad_h3p.  No fp32 dy is written. */
int srpde_bn_bwd_apply_split(const float* y, int ldy, const float* da, int ldda, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, const float* m1,
                             const float* m2, long long P, int C, int flags, const unsigned* dy_amax, void* planes,
                             hipStream_t stream);
int srpde_bn_relu_bwd(const float* y, int ldy, const float* da, int ldda, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, float* dy, int lddy, float* dgamma, float* dbeta,
                      float* dbias, long long P, int C, int relu, unsigned* amax, void* workspace,
                      size_t ws_bytes, hipStream_t stream);

/* ---- input staging: NCHW model input -> NHWC (channel-padded) ----------------------- */
int srpde_nchw_to_nhwc(const float* x, float* out, int n, int cin, int h, int w, int cpad, hipStream_t stream);
/* the way back for the gradient w.r.t. the model input: rows [P, ldx] -> NCHW [n, c, h, w] */
int srpde_nhwc_to_nchw(const float* x, int ldx, float* out, int n, int c, int h, int w, hipStream_t stream);
/* y[:, ch] += alpha * x for y NCHW [n, c, hw], x [n, hw] (the residual path of models.py:74,101) */
int srpde_axpy_channel(float* y, const float* x, int n, int c, int hw, int ch, float alpha, hipStream_t stream);

/* ---- nn.MaxPool2d(2)  (src/models.py:69, used :79-80) -------------------------------- */
int srpde_maxpool2x2_fwd(const float* x, int ldx, float* out, int ldo, int n, int h, int w, int c,
                         hipStream_t stream);
int srpde_maxpool2x2_bwd(const float* x, int ldx, const float* dout, int lddo, float* dx, int lddx, int n, int h,
                         int w, int c, int accumulate, hipStream_t stream);

/* ---- PDEDataset assembly (src/models.py:132-207; replaces the per-field normalisation,
 *      F.interpolate(size=fine, bilinear, align_corners=True) of the coarse field and the
 *      torch.cat of models.py:155-203) -------------------------------------------------
 * u_coarse [n][hc][wc], u_fine / theta_fine / f_fine [n][hf][wf] (contiguous fp32);
 * stats = device {u_mean, u_std, f_mean, f_std, theta_mean, theta_std} (fp32, the split's
 * statistics; theta's ignored when theta_constant != 0, theta then passes through unnormalised).
 * Writes inputs [n][3][hf][wf] = (resize((u_coarse - u_mean) / u_std), theta_n, f_n) and
 * targets [n][1][hf][wf] = (u_fine - u_mean) / u_std. */
int srpde_pde_dataset_assemble(const float* u_coarse, const float* u_fine, const float* theta_fine,
                               const float* f_fine, const float* stats, int theta_constant, int n, int hc, int wc,
                               int hf, int wf, float* inputs, float* targets, hipStream_t stream);

/* ---- batched cascade levels: E examples side by side (src/resolution_comparison.py:160-229 run per example
 *      by src/resolution_comparison_statistical.py:98-205).  Fields are contiguous fp64 [E][n][n] device arrays,
 *      model tensors contiguous fp32 NCHW.  Tiles are ordered example-major, then row-major over the
 *      (S / tile)^2 tiles of one example.  stats = [E][6] fp32 rows {u_mean, u_std, f_mean, f_std, theta_mean,
 *      theta_std}.  All reductions run in a fixed order without atomics: results are bit-reproducible. -------- */
/* GlobalNormalization (resolution_comparison.py:160-181) of every example from the next level's ground truth
 * u / f / theta [E][S2][S2]: mean and unbiased std of the fp32-cast values, accumulated in fp64 and rounded once
 * to fp32.  theta_const[e] (int32) = 1 when theta's fp32 std < 1e-6; that row then holds theta_mean = 0,
 * theta_std = 1, so normalising theta with the row is an exact identity.  The decision stays on the device (no
 * host synchronisation).  Two launches; workspace: srpde_cascade_level_stats_workspace_size bytes, 8-byte aligned. */
size_t srpde_cascade_level_stats_workspace_size(int E, int S2);
int srpde_cascade_level_stats(const double* u, const double* f, const double* theta, int E, int S2, float* stats,
                              int* theta_const, void* workspace, size_t ws_bytes, hipStream_t stream);
/* The U-Net input of one level, x [E (S/tile)^2][3][2 tile][2 tile]: channel 0 = the tile^2 tile of u_cur
 * [E][S][S] cast to fp32, normalised (v - u_mean) / u_std and resized bilinearly (align_corners=True,
 * srpde_upsample_bilinear_fwd's expression) to (2 tile)^2; channels 1 / 2 = the matching tiles of theta_next /
 * f_next [E][2S][2S], normalised.  Bit for bit the torch chain cast, subtract, divide, upsample, cat run per
 * example with the same statistics.  S must be a multiple of tile. */
int srpde_cascade_level_assemble(const double* u_cur, const double* f_next, const double* theta_next,
                                 const float* stats, int E, int S, int tile, float* x, hipStream_t stream);
/* The way back: u_next [E][2S][2S] fp64 = y * u_std + u_mean (an fp32 multiply, then an fp32 add, widened) of
 * the U-Net output y [E (S/tile)^2][1][2 tile][2 tile], every tile at its place.  S is the level's INPUT size, as
 * in srpde_cascade_level_assemble. */
int srpde_cascade_stitch_denorm(const float* y, const float* stats, int E, int S, int tile, double* u_next,
                                hipStream_t stream);
/* Error metrics per example (resolution_comparison_statistical.py:171-178): out [E][3] fp64 = {mean |d|,
 * sqrt(mean d^2), max |d|}, d = pred - gt in fp64; pred [E][n][n] is fp32 (pred_is_f32 != 0) or fp64, gt fp64.
 * Two launches; workspace: srpde_field_metrics_workspace_size bytes, 8-byte aligned. */
size_t srpde_field_metrics_workspace_size(int E, int n);
int srpde_field_metrics(const void* pred, int pred_is_f32, const double* gt, int E, int n, double* out,
                        void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- overlapping-tile cascade levels (ABI 16): the batched cascade above for a user's own fields.  Windows of
 *      tile^2 coarse points overlap and are blended with a partition of unity, so tile borders are no seams and S
 *      need not be a multiple of the tile; the statistics come from the level's inputs, not from its ground truth.
 *      Geometry, the same on both axes: window k of m = ceil((S - tile) / stride) + 1 starts at
 *      start_k = min(k stride, S - tile) on the coarse grid and covers [2 start_k, 2 start_k + 2 tile) on the fine
 *      grid.  Valid: 1 <= stride <= tile <= S <= 16384 and E m^2 within an int.  Tiles are ordered example-major,
 *      then row-major over the m x m windows.  Fields, stats and model tensors as in the section above.
 *      Measured on one MI355X (profiles/tiled_inference_bench.json; E = 10, S = 320, tile 20, stride 10, 9610
 *      windows): statistics 21 us, assemble 98 us, blend 35 us; the whole 40 -> 640 cascade 92.0 ms per call
 *      against 27.4 ms with disjoint tiles, the U-Net forwards being the rest. -------- */
/* m for a geometry; a negative code (-2) with a message for an invalid one.  Host only. */
int srpde_tiled_tiles_per_side(int S, int tile, int stride);
/* The stats rows and theta_const flags of srpde_cascade_level_stats, from what the level is given: {u_mean, u_std}
 * from u_cur [E][S][S], the f and theta columns from f_next / theta_next [E][2S][2S].  Every field is reduced with
 * the partition and order srpde_cascade_level_stats uses for a field of its own length, so the u columns are
 * bit-equal to srpde_cascade_level_stats(u_cur, u_cur, u_cur, E, S) and the others to
 * srpde_cascade_level_stats(f_next, f_next, theta_next, E, 2S).  Two launches, no atomics; workspace:
 * srpde_tiled_level_stats_workspace_size(E, S) bytes, 8-byte aligned. */
size_t srpde_tiled_level_stats_workspace_size(int E, int S);
int srpde_tiled_level_stats(const double* u_cur, const double* f_next, const double* theta_next, int E, int S,
                            float* stats, int* theta_const, void* workspace, size_t ws_bytes, hipStream_t stream);
/* The U-Net input x [E m^2][3][2 tile][2 tile]: srpde_cascade_level_assemble's expressions element for element with
 * the window origin at start_k, so tile (e, i, j) is bit-equal to srpde_cascade_level_assemble run on the fields
 * cropped to that window.  With stride == tile and S a multiple of tile the whole output equals it. */
int srpde_tiled_assemble(const double* u_cur, const double* f_next, const double* theta_next, const float* stats,
                         int E, int S, int tile, int stride, float* x, hipStream_t stream);
/* The way back: per pixel of u_next [E][2S][2S] fp64, over the windows that cover it in ascending tile order,
 * num = sum w (double)y (fp64) and den = sum w (integer); v = num / den rounded once to fp32; u_next = v * u_std +
 * u_mean as in srpde_cascade_stitch_denorm (an fp32 multiply, then an fp32 add, widened).  w = w1(y) w1(x) at the
 * pixel's position inside the window: window = 0 ("linear") w1(i) = min(i + 1, 2 tile - i), window = 1 ("flat")
 * w1(i) = 1.  Every product w y is exact in fp64, so a pixel under one window gets that window's value unchanged
 * (stride == tile: srpde_cascade_stitch_denorm bit for bit) and windows that agree blend to the value they agree
 * on.  Gather form, one launch, no atomics: bit-reproducible. */
int srpde_tiled_blend_denorm(const float* y, const float* stats, int E, int S, int tile, int stride, int window,
                             double* u_next, hipStream_t stream);

/* ---- bicubic, align_corners=True, single-channel fields [planes][h][w] -> [planes][ho][wo]:
 *      F.interpolate(mode='bicubic') of the cascade's interpolation baselines
 *      (src/resolution_comparison_enhanced.py:43-65 multi-level, :386-392 direct) --------- */
int srpde_resize_bicubic_ac(const float* x, float* out, int planes, int h, int w, int ho, int wo,
                            hipStream_t stream);

/* ---- bilinear, align_corners=True: nn.Upsample(2) (models.py:70, :89-93) and the
 *      F.interpolate(size=(40,40)) of PDEDataset (models.py:182-187) ------------------ */
int srpde_upsample_bilinear_fwd(const float* x, int ldx, float* out, int ldo, int n, int h, int w, int ho, int wo,
                                int c, hipStream_t stream);
int srpde_upsample_bilinear_bwd(const float* dout, int lddo, float* dx, int lddx, int n, int h, int w, int ho,
                                int wo, int c, int accumulate, hipStream_t stream);
/* srpde_upsample_bilinear_bwd of (dout + dsa (x) wg): the attention gating gradient
 * dg[q][c] += dsa[q] * wg[c] (models.py:116, srpde_att_bwd called with dg == NULL leaves dsa in
 * workspace[0, P)) folded into the upsample backward that consumes dg (models.py:89,92), so the
 * gating gradient is never written.  Needs c / 4 a power of two <= 256. */
/* srpde_upsample_bilinear_fwd that also forms the spatial attention of the gate reading the result
 * (models.py:124-125, 89/92): sa[q] = sigmoid(sum_c wg[c] out[q][c] + bg[0]).  c / 4 a power of two
 * <= 64.  With srpde_att_channel_fwd's ca, srpde_att_apply_fwd then finishes the gate. */
int srpde_upsample_bilinear_gate_fwd(const float* x, int ldx, float* out, int ldo, int n, int h, int w, int ho,
                                      int wo, int c, const float* wg, const float* bg, float* sa, hipStream_t stream);
/* The spatial attention of the gate whose gating input is up(x) (srpde_upsample_bilinear_gate_fwd's sa),
 * from the low-resolution x alone: sa[q] = sigmoid(up(x . wg)[q] + bg[0]) -- the 1x1 conv commutes with
 * the bilinear upsample, so up(x) need not exist (the decoder conv reads it through srpde_conv_fwd_h3's
 * x0_up).  Equal to the materialised form up to fp32 rounding.  workspace: n h w floats. */
size_t srpde_upsample_gate_sa_workspace_size(int n, int h, int w);
int srpde_upsample_gate_sa(const float* x, int ldx, int n, int h, int w, int ho, int wo, int c, const float* wg,
                           const float* bg, float* sa, void* workspace, size_t ws_bytes, hipStream_t stream);
/* The output head in inference, one pass (models.py:59-61, 98-101, eval mode): out[p] =
 * final(relu(bn2(out_conv2(z))))[p] + xin[n][0][q], z = [n h w][32] (row stride ldz) with its max|z|
 * word, out_conv2's h3 forward planes [2][16][288] / wexp[16] (srpde_split_weights_h3) and bias,
 * out_bn2's eval constants (srpde_bn_eval_prepare's mean / invstd, gamma, beta), final's weight [16] /
 * bias [1], xin the U-Net input (NCHW, xin_c channels).  out_conv2's values equal the h3 kernels';
 * the 16-channel dot sums in another order than srpde_head_fwd.  Replaces srpde_conv_fwd_h3 (out_conv2,
 * ep_*) + srpde_head_fwd.  Needs w <= 63. */
/* 1 if srpde_conv_head_eval takes images of width w (its halo tile needs w <= 63), else 0: wider images
 * run out_conv2 on srpde_conv_fwd_h3 and the head separately. */
int srpde_conv_head_eval_supported(int w);
int srpde_conv_head_eval(const float* z, int ldz, const unsigned* amax_z, const void* wsplit, const int* wexp,
                         const float* bias, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                         const float* bn_beta, const float* wf, const float* bf, const float* xin, int xin_c, int n,
                         int h, int w, float* out, hipStream_t stream);
/* out[p][c] = x[p][c] * ca[n][c] * sa[p] (models.py:122, 128) */
int srpde_att_apply_fwd(const float* x, int ldx, int n, int hw, int c, const float* ca, const float* sa, float* out,
                        int ldo, hipStream_t stream);
int srpde_upsample_bilinear_bwd_gated(const float* dout, int lddo, const float* dsa, const float* wg, float* dx,
                                      int lddx, int n, int h, int w, int ho, int wo, int c, int accumulate,
                                      hipStream_t stream);
/* The same (accumulate = 0) with the backward reduction of the BatchNorm (+ ReLU, flags SRPDE_BN_RELU) whose
 * output gradient dx is -- the decoder block below the upsample (dec2.bn2 under u2, dec3.bn2 under u3,
 * models.py:88-93): y its pre-BN input, mean / invstd the batch statistics; part receives [n*h][c] float2
 * partials (sum dz, sum dz*xhat) and da_max[n*h] max|dx| per input row, the (part, da_max) pair
 * srpde_bn_bwd_prepare / srpde_bn_relu_bwd_part take, so the BN backward does not re-read dx.  Shapes:
 * srpde_upsample_bwd_bn_supported (the row-blocked kernel). */
/* The attention gate's gating gradient dg[p][c] += dsa[p] * wg[c] (srpde_att_bwd's dg pass, called with dg = NULL
 * to leave it out) fused with the backward reduction of the BN (+ ReLU) whose output gradient dg is -- the
 * bridge's last BN under att3's gating signal (models.py:46-48, 88): part [srpde_gating_bn_reduce_blocks][C]
 * float2 and da_max[blocks], the pair srpde_bn_bwd_prepare / srpde_bn_relu_bwd_part take.  C / 4 divides 256. */
int srpde_gating_bn_reduce_blocks(long long P, int C);
int srpde_gating_bn_reduce(const float* dsa, const float* wg, float* dg, int lddg, const float* y, int ldy,
                           const float* mean, const float* invstd, const float* gamma, const float* beta, long long P,
                           int C, int flags, void* part, float* da_max, hipStream_t stream);
int srpde_upsample_bwd_bn_supported(int h, int w, int ho, int wo, int c, int lddo, int lddx);
int srpde_upsample_bilinear_bwd_gated_bn(const float* dout, int lddo, const float* dsa, const float* wg, float* dx,
                                         int lddx, int n, int h, int w, int ho, int wo, int c, const float* y, int ldy,
                                         const float* mean, const float* invstd, const float* gamma,
                                         const float* beta, int flags, void* part, float* da_max,
                                         hipStream_t stream);

/* ---- AttentionGate.forward / backward (src/models.py:103-130) ----------------------- */
int srpde_att_fwd(const float* x, int ldx, const float* g, int ldg, int n, int hw, int c, int gc, const float* w1,
                  const float* b1, const float* w2, const float* b2, const float* wg, const float* bg, float* m,
                  float* hbuf, float* ca, float* sa, float* out, int ldo, hipStream_t stream);
/* srpde_att_fwd in two halves: the channel attention (mean over the pixels, the two 1x1 convs,
 * sigmoid -> ca [n][c]; depends on x alone, so it may run as soon as x exists, on another stream)
 * and the gate (spatial attention of g -> sa [n*hw], out = x * ca * sa). */
int srpde_att_channel_fwd(const float* x, int ldx, int n, int hw, int c, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* m, float* hbuf, float* ca, hipStream_t stream);
int srpde_att_gate_fwd(const float* x, int ldx, const float* g, int ldg, int n, int hw, int c, int gc,
                       const float* ca, const float* wg, const float* bg, float* sa, float* out, int ldo,
                       hipStream_t stream);
/* c a multiple of 32 in 32..1024, gc a multiple of 4 in 4..1024: the size query returns 0 for other counts and
 * srpde_att_bwd, srpde_att_bwd_params and srpde_att_bwd_params_lowres reject them. */
size_t srpde_att_bwd_workspace_size(int n, int hw, int c, int gc);
/* dg == NULL: the gating gradient is not written; workspace[0, n*hw) floats then holds dsa (the
 * spatial gate's pre-sigmoid gradient) for srpde_upsample_bilinear_bwd_gated. */
int srpde_att_bwd(const float* dout, int lddo, const float* x, int ldx, const float* g, int ldg, int n, int hw,
                  int c, int gc, const float* w1, const float* w2, const float* wg, const float* m, const float* hbuf,
                  const float* ca, const float* sa, float* dx, int lddx, int dx_accumulate, float* dg, int lddg,
                  int dg_accumulate, float* dw1, float* db1, float* dw2, float* db2, float* dwg, float* dbg,
                  void* workspace, size_t ws_bytes, hipStream_t stream);
/* dx == NULL: the input gradient is not formed here -- workspace + n*hw floats then holds dm [n][c] (the
 * channel branch's term) for srpde_att_pool_bn_bwd. */
/* The gradient of an encoder block's output e = relu(bn(y)) that feeds both an AttentionGate (its x) and a 2x2
 * max-pool (models.py:79-80, 90/93, 119-130), and that BatchNorm's backward reduction, in one pass: de = (dout * sa)
 * * ca + dm (srpde_att_bwd's input gradient; dm from the srpde_att_bwd call with dx == NULL) plus dp [n*h/2*w/2][c]
 * routed to each 2x2 window's first maximum of a (= e; srpde_maxpool2x2_bwd's choice), written once -- bit for bit
 * srpde_att_bwd(dx) + srpde_maxpool2x2_bwd(accumulate); part [srpde_att_pool_bn_bwd_blocks()][c] float2 receives
 * (sum dz, sum dz*xhat) per block (dz = de * [bn output > 0], xhat from y, mean, invstd, gamma, beta as in
 * srpde_bn_relu_bwd) and da_max[block] max|de|: the `part` / `da_max` of srpde_bn_bwd_prepare, which then makes no
 * pass over y and de of its own.  c / 4 a power of two <= 64; h, w even. */
int srpde_att_pool_bn_bwd_blocks(int n, int h, int w, int c);
int srpde_att_pool_bn_bwd(const float* dout, int lddo, const float* ca, const float* sa, const float* dm, const float* a,
                          int lda, const float* dp, int lddp, const float* y, int ldy, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, float* de, int ldde, int n, int h,
                          int w, int c, void* part, float* da_max, hipStream_t stream);
/* The parameter-gradient half of srpde_att_bwd (dW1, db1, dW2, db2 of the channel MLP, dwg, dbg of
 * the spatial gate: fixed-order reductions over samples / pixel blocks of the per-sample rows it
 * left in `workspace`).  srpde_att_bwd with dw1 == NULL stops before it, so a caller can queue
 * these reductions on another stream (nothing downstream in the backward reads them). */
int srpde_att_bwd_params(const float* g, int ldg, int n, int hw, int c, int gc, const float* m, const float* hbuf,
                         float* dw1, float* db1, float* dw2, float* db2, float* dwg, float* dbg, void* workspace,
                         size_t ws_bytes, hipStream_t stream);
/* srpde_att_bwd_params for a gate whose gating input is the bilinear x2 upsample of d ([n*h*w][gc], the decoder
 * block's low-res output, models.py:89 / :92, hw = ho*wo the gate's resolution): the spatial conv's weight
 * gradient sum_p dsa[p] up(d)[p] is formed as sum_q d[q] (up^T dsa)[q] over the low-res rows (4x fewer bytes
 * read; the same sum regrouped, fp32 rounding apart), the bias gradient as sum_q (up^T dsa)[q]. */
int srpde_att_bwd_params_lowres(const float* d, int ldd, int n, int h, int w, int ho, int wo, int c, int gc,
                                const float* m, const float* hbuf, float* dw1, float* db1, float* dw2, float* db2,
                                float* dwg, float* dbg, void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- output head: final 1x1 conv + residual x[:,0:1] (models.py:61,74,98,101) ------- */
int srpde_head_fwd(const float* z, int ldz, int c, const float* wf, const float* bf, const float* xin, int xin_c,
                   int n, int hw, float* out, hipStream_t stream);
/* c a multiple of 4 in 4..1024: the size query returns 0 for other counts and srpde_head_bwd rejects them. */
size_t srpde_head_bwd_workspace_size(int n, int hw, int c);
int srpde_head_bwd(const float* dout, const float* z, int ldz, int c, const float* wf, int n, int hw, float* dz,
                   int lddz, float* dwf, float* dbf, void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- nn.MSELoss (src/train_enhanced.py:70,307) --------------------------------------- */
size_t srpde_mse_workspace_size(void);
int srpde_mse_fwd(const float* y, const float* t, long long n, float* loss, void* workspace, size_t ws_bytes,
                  hipStream_t stream);
int srpde_mse_bwd(const float* y, const float* t, long long n, const float* gout, float* dy, hipStream_t stream);

/* ---- MSE plus the residual of the discrete equation the samples solve (no counterpart in the reference, whose
 *      README lists "physics-informed loss functions that incorporate PDE residuals" as future work) ----------
 * y, t [B][1][n][n] fp32: normalised prediction and target; x [B][3][n][n] fp32 (NCHW): the model input, channel 1
 * theta and channel 2 f as the dataset stores them; stats: 6 floats on the device (u_mean, u_std, f_mean, f_std,
 * theta_mean, theta_std; (0, 1) for a constant theta); kind [B] int32: 0 = whole-domain sample (zero ghost ring, all
 * n^2 nodes counted, 1 / h^2 = inv_h2_std), 1 = crop of a finer solve (the (n - 2)^2 interior nodes counted,
 * 1 / h^2 = inv_h2_sub).  With theta = theta_std x1 + theta_mean, f = f_std x2 + f_mean, A the 5-point stencil with
 * zero outside the grid (A 1 = -(number of missing neighbours)) and m the mask of the counted nodes,
 *     r    = (theta (u_std A y + u_mean A 1) / h^2 - f) / f_std          (fp32, in this split form)
 *     loss = {mse + weight pde, mse, pde},  mse = mean((y - t)^2),  pde = sum(m r^2) / M,  M = sum(m)
 * (fp64 sums in a fixed order: bit-reproducible).  dy_unit (nullable) [B][1][n][n]: the gradient for grad_out = 1,
 *     2 (y - t) / (B n^2) + weight (2 u_std / (M f_std h^2)) A(m r theta)         (h per sample)
 * -- NULL: no gradient is computed or written.  3 <= n <= 64.  Two launches, no atomics, no host sync; workspace:
 * srpde_physics_loss_workspace_size bytes (0 for an unsupported shape), 8-byte aligned.  srpde_physics_loss_bwd:
 * dy = grad_out[0] * dy_unit over count values (grad_out NULL: 1), one launch. */
size_t srpde_physics_loss_workspace_size(int B, int n);
int srpde_physics_loss_fwd(const float* y, const float* t, const float* x, const int* kind, const float* stats, int B,
                           int n, float weight, float inv_h2_std, float inv_h2_sub, float* loss, float* dy_unit,
                           void* workspace, size_t ws_bytes, hipStream_t stream);
int srpde_physics_loss_bwd(const float* dy_unit, long long count, const float* gout, float* dy, hipStream_t stream);
/* The same loss with the residual of the divergence-form equation div(theta grad u) = f (ABI 19; the operator of
 * srpde_div_apply below, face_mean 0 arithmetic / 1 harmonic, in fp32).  Arguments, outputs, kinds and reductions as
 * srpde_physics_loss_fwd.  With a(y) = (cE (yE - y) + cW (yW - y)) + (cS (yS - y) + cN (yN - y)) on y with a zero halo
 * and the ghost coefficient theta_a, and k_miss the number of the node's neighbours outside the grid
 * (D_theta 1 = -k_miss theta exactly: the interior faces cancel),
 *     r = ((u_std a(y) + u_mean (-k_miss theta)) / h^2 - f) / f_std          (fp32, in this split form)
 * dy_unit = 2 (y - t) / (B n^2) + weight (2 u_std / (M f_std h^2)) Dt(m r), Dt the same face sum (symmetric, the
 * ghost faces on its diagonal).  On a kind-1 sample m r is zero on the ring, so the ghost coefficient there is
 * immaterial.  3 <= n <= 64; the kernel's LDS (three halo tiles per sample, 51 KiB at n = 64) stays inside the 64 KiB
 * a kernel may use without raising its limit.  Two launches; workspace: srpde_physics_loss_div_workspace_size bytes
 * (0 for an unsupported shape), 8-byte aligned.  The gradient is scaled by srpde_physics_loss_bwd. */
size_t srpde_physics_loss_div_workspace_size(int B, int n);
int srpde_physics_loss_div_fwd(const float* y, const float* t, const float* x, const int* kind, const float* stats,
                               int B, int n, int face_mean, float weight, float inv_h2_std, float inv_h2_sub,
                               float* loss, float* dy_unit, void* workspace, size_t ws_bytes, hipStream_t stream);
/* How well raw fields satisfy the discrete equation: out [E][2] fp64 = {sqrt(mean r^2), max |r|} per example over
 * the counted nodes (all, or the (n - 2)^2 interior ones with interior_only != 0), r = theta A u inv_h2 - f in fp64
 * with u [E][n][n] fp32 (u_is_f32 != 0) or fp64, f and theta fp64.  r is evaluated as
 * (theta * (((up + down) + (left + right)) - 4 u)) * inv_h2 - f, every operation rounded on its own, so a host
 * restatement in that order reproduces it bit for bit.  Two launches; workspace:
 * srpde_pde_residual_metrics_workspace_size bytes, 8-byte aligned. */
size_t srpde_pde_residual_metrics_workspace_size(int E, int n);
int srpde_pde_residual_metrics(const void* u, int u_is_f32, const double* f, const double* theta, int E, int n,
                               double inv_h2, int interior_only, double* out, void* workspace, size_t ws_bytes,
                               hipStream_t stream);
/* Weighted-Jacobi sweeps of theta * L u = f (csrc/relax.hip, relax_kernel<PointwiseOp>): the smoother that takes the
 * grid-scale error out of a field that is right at low frequencies (a cascade level's output).  u_in, f, theta, u_out
 * [E][n][n] fp64.  One sweep, every operation rounded once in this order (no contraction), from the previous sweep's u
 * throughout:
 *     g  = f / (theta * inv_h2)
 *     s  = (u[y-1][x] + u[y+1][x]) + (u[y][x-1] + u[y][x+1])        a neighbour outside the grid is 0
 *     r  = (s - 4.0 * u) - g
 *     u' = u + (0.25 * omega) * r
 * so a host restatement in that order reproduces the result bit for bit, whatever the tiling.  interior_only != 0
 * (n >= 3): the nodes with y or x in {0, n - 1} keep their input value and only the inner (n - 2)^2 move (a crop
 * whose ring is not zero).  0 < omega <= 1: no error component grows.  A launch does up to
 * srpde_pde_relax_sweeps_per_launch() sweeps on tiles held in LDS; more sweeps alternate between u_out and the
 * workspace (one [E][n][n] fp64 field, srpde_pde_relax_workspace_size bytes, 0 when one launch suffices) so that the
 * last launch writes u_out; sweeps = 0 copies u_in to u_out.  E <= 65535, n <= 16384, pointers 8-byte aligned; u_out
 * must not overlap u_in, f, theta or the workspace.  Stream-ordered, no host sync, no state. */
int srpde_pde_relax_sweeps_per_launch(void);
size_t srpde_pde_relax_workspace_size(int E, int n, int sweeps);
int srpde_pde_relax(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                    double inv_h2, int sweeps, double omega, int interior_only, void* workspace, size_t ws_bytes,
                    hipStream_t stream);
/* Weighted-Jacobi sweeps of div(theta grad u) = f (csrc/relax.hip, relax_kernel<DivOp>, ABI 19): the same kernel for
 * the operator of srpde_div_apply below (face coefficients cE, cW, cS, cN from face_mean 0 arithmetic / 1 harmonic,
 * c = theta_a and u_b = 0 towards the ghost ring; E is x + 1, S is y + 1).  One sweep, every operation rounded once in
 * this order (no contraction), from the previous sweep's u throughout:
 *     once per node:  g = f / inv_h2
 *                     w = omega / ((cE + cW) + (cS + cN))
 *     per sweep:      a  = (cE*(uE - u) + cW*(uW - u)) + (cS*(uS - u) + cN*(uN - u))
 *                     u' = u + w * (a - g)
 * so a host restatement in that order reproduces the result bit for bit, whatever the tiling or the launch split.
 * The error operator is I - omega diag(-D_theta)^-1 (-D_theta); -D_theta is a symmetric, weakly diagonally dominant
 * M-matrix, so for 0 < omega <= 1 no error component grows.  interior_only, the workspace, the limits, the alignment
 * and the overlap rules are those of srpde_pde_relax; srpde_pde_relax_sweeps_per_launch() answers for both. */
size_t srpde_div_relax_workspace_size(int E, int n, int sweeps);
int srpde_div_relax(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                    int face_mean, double inv_h2, int sweeps, double omega, int interior_only, void* workspace,
                    size_t ws_bytes, hipStream_t stream);

/* ---- clip_grad_norm_ + AdamW on one flat buffer (src/train_enhanced.py:74-75,308) ---- */
size_t srpde_grad_norm_workspace_size(void);
int srpde_clip_coef(const float* g, long long n, float grad_scale, float max_norm, float* coef, void* workspace,
                    size_t ws_bytes, hipStream_t stream);
int srpde_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int step, const float* coef, float grad_scale,
                     hipStream_t stream);

/* ---- Poisson: replaces scipy.sparse.linalg.spsolve(diag(theta) @ L, f)
 *      (src/data_generation.py:79-104, src/enhanced_data_generation.py:47-68) -------- */
int srpde_poisson_lds_max_n(void);
/* forcing f = sin(2 pi k1 X) sin(2 pi k2 Y) for B (k1, k2) pairs on linspace(0,1,n)^2
 * (PoissonSolver.generate_forcing_term, src/data_generation.py:60-77) */
int srpde_forcing_batched(const double* k12, int B, int n, double* out, hipStream_t stream);
size_t srpde_poisson_workspace_size(int B, int n);
/* The batched solve in one call (replaces spsolve(diag(theta) @ L, f), data_generation.py:79-104,
 * for B problems at once): f, theta, u are [B][n][n] fp64 device arrays, iters_out [B] int32
 * (nullable; -1 marks a problem whose cooperative launch aborted at a stuck grid barrier).
 * n <= srpde_poisson_lds_max_n(): one stream-ordered launch, no workspace.  Larger n: grid CG with
 * workspace (srpde_poisson_workspace_size bytes), run as cooperative launches (Chronopoulos-Gear CG,
 * one grid barrier per iteration, block size chosen per (B, n)) -- stream-ordered, the host never
 * waits.  Only when srpde_poisson_coop_problems(n) is 0 (n > 1024) the call drives the split entry
 * points below (textbook CG) and polls convergence every 128 iterations, synchronising `stream`.
 * Magnitude range: the solve is equivariant under scaling of f (by a power of two: bit for bit, iteration counts
 * included) while gamma0 = |f / theta|^2 summed over the grid and rtol^2 gamma0, where the iteration stops, are
 * normal fp64 numbers, and delta0 <= 8 (n - 1)^2 gamma0 finite -- for rtol = 1e-12 and n <= 1024 about
 * 2^-470 < |f / theta| < 2^490 per node.  (The Chronopoulos-Gear
 * scalars are formed from inner products scaled by the power of two of gamma0's exponent, so no product of them
 * leaves the range before gamma itself does.)  Outside it, and for non-finite f or theta <= 0, u is undefined. */
int srpde_poisson_cg_batched(const double* f, const double* theta, double* u, int B, int n, double rtol, int maxit,
                             int* iters_out, void* workspace, size_t ws_bytes, hipStream_t stream);
/* (Test hook: rtol < 0 solves to |rtol| but every cooperative grid-CG launch starts aborted -- iters_out = -1 for
 * its problems, u undefined -- to exercise a caller's handling of a stuck grid barrier; poisson.solve_batched
 * raises.  The LDS solver, n <= srpde_poisson_lds_max_n(), has no barrier to abort.) */
/* Problems per cooperative grid-CG launch at this n with its largest (8192-point) blocks; 0 when one
 * problem does not fit the co-resident grid or n > 1024 (a block's two halo rows, the neighbours'
 * edge rows, take at most two points per thread). */
int srpde_poisson_coop_problems(int n);
int srpde_poisson_cg_lds(const double* f, const double* theta, double* u, int B, int n, double rtol, int maxit,
                         int* iters, double* resid, hipStream_t stream);
int srpde_poisson_cg_grid_init(const double* f, const double* theta, int B, int n, void* ws, size_t ws_bytes,
                               hipStream_t stream);
int srpde_poisson_cg_grid_iterate(int B, int n, double rtol, int k_begin, int k_count, int maxit, void* ws,
                                  size_t ws_bytes, hipStream_t stream);
size_t srpde_poisson_cg_grid_done_offset(int B, int n);
int srpde_poisson_cg_grid_finish(double* u, int* iters, int B, int n, int maxit, void* ws, size_t ws_bytes,
                                 hipStream_t stream);

/* ---- Direct Poisson solve by the 2-D sine transform (DST-I): the same system as srpde_poisson_cg_batched,
 *      solved exactly.  L = (T (x) I + I (x) T) / h^2 with T = tridiag(1, -2, 1); the symmetric orthogonal
 *      S[j][k] = sqrt(2 / (n + 1)) sin(pi (j + 1)(k + 1) / (n + 1)) diagonalises T with eigenvalues
 *      lam_k = -4 sin^2(pi (k + 1) / (2 (n + 1))), so
 *          U = S ( (S (F / Theta) S) o h^2 / (lam_i + lam_j) ) S
 *      -- four dense fp64 products against one matrix per problem (fp64 MFMA): no iteration, no cooperative
 *      launch, no grid barrier, any n up to 16384.  Results are bit-reproducible and independent of B. ---- */
/* The plan is a caller-owned device buffer (the library keeps no state): S [n][n] then lam [n], fp64.
 * A plan belongs to one n; the solve entries take it with its exact size, srpde_poisson_dst_plan_size(n)
 * bytes (0 for an n outside 1 .. 16384), and refuse any other size. */
size_t srpde_poisson_dst_plan_size(int n);
/* Fills the plan for n (one launch; plan_bytes >= srpde_poisson_dst_plan_size(n), plan 8-byte aligned). */
int srpde_poisson_dst_plan(int n, void* plan, size_t plan_bytes, hipStream_t stream);
/* n up to which one workgroup solves one problem with S and the field in LDS (one launch, no workspace). */
int srpde_poisson_dst_lds_max_n(void);
/* Workspace of the two entries below: 0 for n <= srpde_poisson_dst_lds_max_n() (and for B <= 0), else one
 * [B][n][n] fp64 field; 16-byte aligned. */
size_t srpde_poisson_dst_workspace_size(int B, int n);
/* u = solution of theta * L u = f for B problems: f, theta, u are [B][n][n] fp64 device arrays, n >= 2.
 * Above the LDS limit: four launches of a batched tiled product (f / theta at the first one's load, the
 * eigenvalue scaling at the second one's store); u must not alias f or theta there.  Stream-ordered, no host
 * sync, no state: capturable in a graph. */
int srpde_poisson_dst_batched(const double* f, const double* theta, double* u, int B, int n, const void* plan,
                              size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream);
/* y = S x S, the orthonormal 2-D DST-I of B fields [B][n][n] (its own inverse); y must not alias x above the
 * LDS limit. */
int srpde_poisson_dst_apply(const double* x, double* y, int B, int n, const void* plan, size_t plan_bytes, void* ws,
                            size_t ws_bytes, hipStream_t stream);

/* ---- Divergence-form operator D_theta u = div(theta grad u) (csrc/poisson_div.hip): the conservative
 *      variable-coefficient problem, beside theta * L u = f of every entry above.  Same grid (all n^2 nodes unknown,
 *      a zero ghost ring, h = 1 / (n - 1)).  For node a with nodal theta_a and neighbour b the face coefficient is
 *          face_mean 0 (arithmetic):  c = 0.5 * (ta + tb)
 *          face_mean 1 (harmonic):    c = (2.0 * (ta * tb)) / (ta + tb)
 *          b outside the grid:        c = ta, u_b = 0
 *      and, every operation rounded once in this order (no contraction),
 *          y = ((cE*(uE - u) + cW*(uW - u)) + (cS*(uS - u) + cN*(uN - u))) * inv_h2
 *      so a host restatement in that order reproduces y bit for bit, whatever the tiling.  c is bit-symmetric in
 *      (a, b): D_theta is exactly symmetric, negative definite, and theta * L for a constant theta. ---- */
/* y = D_theta u for B fields: u, theta, y [B][n][n] fp64, 1 <= B <= 65535, 2 <= n <= 16384, pointers 8-byte
 * aligned, y must not alias u or theta; inv_h2 > 0 ((n - 1)^2 for the whole-domain operator).  One launch. */
int srpde_div_apply(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                    hipStream_t stream);
/* D_theta u = f by CG preconditioned with the sine-transform solve of L (srpde_poisson_dst_*, the caller's plan for
 * n): cond(L^-1 D_theta) <= theta_max / theta_min for every n, so the iteration count does not grow with n.  B
 * independent problems; per iteration three streaming launches and the sine-transform solve -- no atomics, no
 * cooperative launch, no grid barrier, no host sync; all sums in a fixed order, so a problem's result is the same
 * bits whatever B is and wherever it stands in the batch.  inv_h2 = (n - 1)^2.
 *   init     x = 0, r = f, z = L^-1 r; a problem with |f| = 0 is done at once (u = 0, iters = 0, resid = 0)
 *   iterate  iterations k_begin .. k_begin + k_count - 1; iterations count from 1 and successive calls continue
 *            where the last one stopped (k_begin = 1, then 1 + k_count, ...), with the same theta, face_mean and
 *            rtol.  A problem is done once |r| <= rtol |f|; it is then frozen -- x, r, p, its iteration count and
 *            residual no longer change and no 0/0 is formed -- so further iterations are harmless and a batch's
 *            results do not depend on its slowest member
 *   finish   u [B][n][n], iters [B] int32 (iterations performed; nullable), resid [B] fp64 (|r| / |f| at the last
 *            one, 0 for f = 0; nullable).  May be called after any iterate; the caller decides when to stop.
 * The int32 vector [B] at byte srpde_div_cg_done_offset of the workspace holds each problem's done flag, valid after
 * init (poll it every few iterations, or never: a fixed iteration count needs no host read and is capturable in a
 * graph).  Workspace: srpde_div_cg_workspace_size bytes (0 for a bad shape), 16-byte aligned, kept by the caller
 * from init to finish; no other state. */
size_t srpde_div_cg_workspace_size(int B, int n);
size_t srpde_div_cg_done_offset(int B, int n);
int srpde_div_cg_init(const double* f, int B, int n, const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                      hipStream_t stream);
int srpde_div_cg_iterate(const double* theta, int B, int n, int face_mean, double rtol, int k_begin, int k_count,
                         const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream);
int srpde_div_cg_finish(double* u, int* iters, double* resid, int B, int n, void* ws, size_t ws_bytes,
                        hipStream_t stream);
/* The same CG from an initial guess (ABI 20), in place of srpde_div_cg_init and on the same workspace: x = u0,
 * r = f - D_theta u0 (D_theta u0 in the rounding order of srpde_div_apply with inv_h2 = (n - 1)^2, then one
 * subtraction), z = L^-1 r; |f| and |r0| are kept apart, so resid stays |r| / |f| and a problem whose u0 already has
 * |r0| <= rtol |f| is done with iters = 0 and u = u0.  |f| = 0: u = 0, iters = 0, resid = 0, whatever u0 is.
 * srpde_div_cg_iterate (k_begin = 1, the same theta, face_mean and rtol) and srpde_div_cg_finish follow unchanged;
 * freezing, batch independence and the absence of host syncs are theirs.  For u0 = 0 and rtol < 1 every bit of u,
 * iters and resid is the zero start's (D 0 = +0, f - 0 = f).  f, u0, theta [B][n][n] fp64, 8-byte aligned; rtol >= 0.
 * One fused launch, the sine-transform solve, one small launch. */
int srpde_div_cg_init_from(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                           double rtol, const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes,
                           hipStream_t stream);
/* The pair gradient of D_theta (ABI 20): g_out = scale * G(u, lam; theta) with
 *     G_a = inv_h2 * sum over b in E, W, S, N of a of  d_ab * (u_b - u_a) * (lam_b - lam_a)
 * where d_ab = dc_ab / dtheta_a is
 *     face_mean 0 (arithmetic):  0.5
 *     face_mean 1 (harmonic):    (2.0 * (tb * tb)) / ((ta + tb) * (ta + tb))
 *     b outside the grid:        1, u_b = lam_b = 0
 * Summing <lam, D_theta u> by parts gives -inv_h2 * (sum over faces of c (u_b - u_a) (lam_b - lam_a)), so
 * d<lam, D_theta u> / dtheta = -G, and with D_theta symmetric
 *     y = D_theta u, upstream gy:      grad_u = D_theta gy,                 grad_theta = -G(u, gy)    (scale -1)
 *     u = D_theta^-1 f, upstream gu:   lam = D_theta^-1 gu,  grad_f = lam,  grad_theta = +G(u, lam)   (scale +1)
 * Every operation is rounded once, in this order (no contraction): a face term is (d_ab * (u_b - u_a)) *
 * (lam_b - lam_a), the four are summed as (E + W) + (S + N), then * inv_h2, then * scale -- a host restatement in
 * that order reproduces g_out bit for bit, whatever the tiling and whatever B.  A gather (no atomics), one launch for
 * all of B.  u, lam, theta, g_out [B][n][n] fp64, shapes and alignment as srpde_div_apply; lam may be u; g_out must
 * not alias an input; inv_h2 > 0 and scale finite. */
int srpde_div_theta_grad(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                         int face_mean, double inv_h2, double scale, hipStream_t stream);

/* ---- The shifted operator A = D_theta - sigma I, sigma >= 0 and finite (ABI 21): the operator of an implicit time
 *      step of u_t = div(theta grad u) - f (sigma = 1 / dt) and of the screened problem (D_theta - sigma) u = f.  A is
 *      as symmetric and negative definite as D_theta.  With M = L - sigma_p I, which the sine transform diagonalises
 *      as it does L, and sigma_p = sigma / theta_g for any theta_g in [theta_min, theta_max],
 *          min(theta_min, theta_g) (-M) <= -A <= max(theta_max, theta_g) (-M)
 *      (from theta_min (-L) <= -D_theta <= theta_max (-L)), so cond(M^-1 A) <= theta_max / theta_min for every n and
 *      every sigma: the CG above, with M as its preconditioner, needs no more iterations than the unshifted solve.
 *      Every entry here with sigma = 0 (and sigma_p = 0) launches the kernels of its unshifted namesake. ---- */
/* y = D_theta u - sigma * u: the y of srpde_div_apply (the face sum, * inv_h2), then the one product sigma * u, then
 * the one subtraction, each rounded once (no contraction).  Arguments as srpde_div_apply.  One launch, the same
 * kernel: the shift is applied where y is stored. */
int srpde_div_apply_shift(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                          double sigma, hipStream_t stream);
/* u = solution of (L - sigma_p I) u = f for B problems, L the 5-point Laplacian of srpde_poisson_dst_batched (no
 * theta): f, u [B][n][n] fp64, n >= 2, sigma_p >= 0 and finite; plan and workspace as srpde_poisson_dst_batched (the
 * plan format is the same).  The eigenvalue scaling h^2 / (lam_i + lam_j) becomes
 *     1 / ((lam_i + lam_j) * inv_h2 - sigma_p),   inv_h2 = (n - 1)^2
 * each operation rounded once in this order (no contraction): the sum of the two eigenvalues, the product with inv_h2,
 * the subtraction, the reciprocal; the transformed field is then multiplied by it -- in the LDS kernel after its
 * second product, above srpde_poisson_dst_lds_max_n() at the second launch's store.  sigma_p = 0 runs the unshifted
 * kernels: the bits of srpde_poisson_dst_batched with theta = 1. */
int srpde_poisson_dst_shift_batched(const double* f, double* u, int B, int n, double sigma_p, const void* plan,
                                    size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream);
/* (D_theta - sigma I) u = f by the CG of srpde_div_cg_*, preconditioned with the sine-transform solve of
 * L - sigma_p I, on the same workspace (srpde_div_cg_workspace_size, srpde_div_cg_done_offset) and finished by
 * srpde_div_cg_finish.  init_shift: x = 0, r = f, z = M^-1 r (r does not depend on sigma).  init_from_shift: x = u0,
 * r = f - (D_theta u0 - sigma * u0) in one fused pass -- the operator in the rounding order of srpde_div_apply_shift
 * with inv_h2 = (n - 1)^2, then one subtraction -- otherwise as srpde_div_cg_init_from (u0 = 0 gives the zero start's
 * bits, a u0 within rtol gives iters = 0).  iterate_shift: q = D_theta p - sigma * p in step (a), z = M^-1 r with
 * sigma_p in step (c); the same sigma, sigma_p, theta, face_mean and rtol in every call of one solve.  The freeze rule,
 * the per-problem fixed-order sums, batch independence and the absence of atomics, barriers and host reads are those
 * of srpde_div_cg_iterate: the update, r.z and finish kernels are the same code. */
int srpde_div_cg_init_shift(const double* f, int B, int n, double sigma_p, const void* plan, size_t plan_bytes,
                            void* ws, size_t ws_bytes, hipStream_t stream);
int srpde_div_cg_init_from_shift(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                                 double sigma, double sigma_p, double rtol, const void* plan, size_t plan_bytes,
                                 void* ws, size_t ws_bytes, hipStream_t stream);
int srpde_div_cg_iterate_shift(const double* theta, int B, int n, int face_mean, double sigma, double sigma_p,
                               double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes, void* ws,
                               size_t ws_bytes, hipStream_t stream);
/* The right-hand side of one implicit time step of u_t = D_theta u - f with a forcing constant over the step, for the
 * solve (D_theta - sigma I) u+ = rhs:
 *     cn 0, backward Euler,  (u+ - u) / dt = D_theta u+ - f,                  sigma = 1 / dt:
 *         rhs = f - sigma * u
 *     cn 1, Crank-Nicolson,  (u+ - u) / dt = (D_theta u+ + D_theta u) / 2 - f, sigma = 2 / dt (the equation times 2):
 *         rhs = (2 f - sigma * u) - D_theta u
 * 2 f is exact; D_theta u is srpde_div_apply's y with inv_h2 = (n - 1)^2; the product sigma * u and the subtractions
 * are rounded once each, in the order written (no contraction).  f == NULL is f = 0 (the same operations on 0.0).
 * u, theta, rhs (and f) [B][n][n] fp64, 8-byte aligned; rhs must not alias u, f or theta; sigma >= 0 and finite.  One
 * launch on srpde_div_apply's tiles; backward Euler reads no neighbour. */
int srpde_div_step_rhs(const double* u, const double* f, const double* theta, double* rhs, int B, int n, int face_mean,
                       double sigma, int cn, hipStream_t stream);

/* ---- Zero-flux (Neumann) sides (ABI 22).  Every entry above wraps the grid in a ghost ring that holds 0: four
 *      homogeneous Dirichlet sides.  The entries here take a side mask bc, 0 .. 15:
 *          bit 0  the row 0 side          bit 1  the row n - 1 side
 *          bit 2  the column 0 side       bit 3  the column n - 1 side
 *      A clear bit is the zero ghost ring as above; a set bit is a zero-flux side, du/dn = 0: that side's ghost faces
 *      are missing, i.e. their coefficient is 0 where it was theta_a (the same as a ghost value equal to the edge
 *      node's).  Every other operation, and its place in the rounding orders stated above, is unchanged: a missing
 *      face's term is 0 * (0 - u_a) (and 0 * (0 - u_a) * (0 - lam_a) in the pair gradient, d_ab = 0), so bc = 0 gives
 *      the bits of the unmasked namesake.  h stays 1 / (n - 1), inv_h2 = (n - 1)^2.  The operator stays exactly
 *      symmetric; it is negative definite unless bc = 15, where the constants are its null space: bc = 15 needs
 *      sigma > 0 (and sigma_p > 0) in every solve entry and is refused without.  A, and M = L_bc - sigma_p I (theta = 1,
 *      the same sides), are sums over the same faces with coefficients in [theta_min, theta_max] and 1, so
 *      cond(M^-1 A) <= theta_max / theta_min for every n, sigma and bc, as above. ---- */
/* y = D_theta u - sigma * u with the sides bc: srpde_div_apply_shift's arguments, rounding order and launch (sigma = 0:
 * srpde_div_apply's). */
int srpde_div_apply_bc(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                       double sigma, int bc, hipStream_t stream);
/* srpde_div_step_rhs with the sides bc in Crank-Nicolson's D_theta u (backward Euler reads no neighbour: its rhs does
 * not depend on bc). */
int srpde_div_step_rhs_bc(const double* u, const double* f, const double* theta, double* rhs, int B, int n,
                          int face_mean, double sigma, int cn, int bc, hipStream_t stream);
/* srpde_div_theta_grad with the sides bc: d_ab = 0 towards a zero-flux side (1 towards a ghost-ring side). */
int srpde_div_theta_grad_bc(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                            int face_mean, double inv_h2, double scale, int bc, hipStream_t stream);
/* The separable solve of the constant-coefficient operator with the sides bc, the preconditioner of the CG below:
 * L_bc = (T_y (x) I + I (x) T_x) / h^2 with T tridiagonal, 1 off the diagonal, -2 on it and -1 at a zero-flux end (T_y
 * acts along the rows' index, its ends are bits 0 / 1; T_x along the columns', bits 2 / 3).  T = Q diag(lam) Q^T with,
 * for nodes j and modes k = 0 .. n - 1, unit columns
 *     ring - ring   Q[j][k] = sqrt(2 / (n + 1)) sin(pi (j + 1)(k + 1) / (n + 1)),      lam_k = -4 sin^2(pi (k + 1) / (2 (n + 1)))
 *     ring - flux   Q[j][k] = 2 / sqrt(2 n + 1) sin(pi (j + 1)(2 k + 1) / (2 n + 1)),  lam_k = -4 sin^2(pi (2 k + 1) / (2 (2 n + 1)))
 *     flux - ring   the same with j -> n - 1 - j
 *     flux - flux   Q[j][k] = sqrt((k ? 2 : 1) / n) cos(pi (2 j + 1) k / (2 n)),       lam_k = -4 sin^2(pi k / (2 n))
 * (the trigonometric arguments reduced in integers first), so
 *     U = Q_y ( (Q_y^T F Q_x) o 1 / ((lam_y,i + lam_x,j) * inv_h2 - sigma_p) ) Q_x^T
 * the scaling in the rounding order of srpde_poisson_dst_shift_batched.  Four launches of the batched fp64-MFMA tile
 * product at every n (there is no one-workgroup kernel for mixed sides).
 * The plan is a caller-owned device buffer of doubles: Q_x, Q_x^T, Q_y, Q_y^T ([n][n] each), lam_y [n], lam_x [n], the
 * mask as a double, then bc unused doubles -- so that a plan's size, srpde_poisson_sep_plan_size(n, bc) bytes (0 for a
 * bad n or mask), names both its n and its mask, and every entry refuses a plan made for another of either without
 * reading it back.  Workspace: srpde_poisson_sep_workspace_size(B, n) bytes, one [B][n][n] field, 16-byte aligned. */
size_t srpde_poisson_sep_plan_size(int n, int bc);
int srpde_poisson_sep_plan(int n, int bc, void* plan, size_t plan_bytes, hipStream_t stream);
size_t srpde_poisson_sep_workspace_size(int B, int n);
/* u = solution of (L_bc - sigma_p I) u = f for B problems: f, u [B][n][n] fp64, 8-byte aligned, u must not alias f;
 * n >= 2, sigma_p >= 0 and finite, > 0 for bc = 15.  Stream-ordered, no host sync, no state. */
int srpde_poisson_sep_shift_batched(const double* f, double* u, int B, int n, int bc, double sigma_p, const void* plan,
                                    size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream);
/* (D_theta - sigma I) u = f with the sides bc by the CG of srpde_div_cg_*_shift, preconditioned with the separable
 * solve above (plan: srpde_poisson_sep_plan for n and the same bc).  Arguments, rounding orders, the freeze rule and
 * the per-problem fixed-order sums are the shifted entries'; sigma = sigma_p = 0 is the unshifted problem.  The
 * workspace is srpde_div_cg_workspace_size_bc(B, n) bytes: the layout of srpde_div_cg_workspace_size with the separable
 * solve's field behind it, so srpde_div_cg_done_offset and srpde_div_cg_finish serve these entries too. */
size_t srpde_div_cg_workspace_size_bc(int B, int n);
int srpde_div_cg_init_bc(const double* f, int B, int n, int bc, double sigma_p, const void* plan, size_t plan_bytes,
                         void* ws, size_t ws_bytes, hipStream_t stream);
int srpde_div_cg_init_from_bc(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                              int bc, double sigma, double sigma_p, double rtol, const void* plan, size_t plan_bytes,
                              void* ws, size_t ws_bytes, hipStream_t stream);
int srpde_div_cg_iterate_bc(const double* theta, int B, int n, int face_mean, int bc, double sigma, double sigma_p,
                            double rtol, int k_begin, int k_count, const void* plan, size_t plan_bytes, void* ws,
                            size_t ws_bytes, hipStream_t stream);
/* srpde_div_relax with the sides bc (ABI 23; csrc/relax.hip, relax_kernel<DivOp<HARM, true>>: the same tiles, halo and
 * sweeps per launch).  Only the face coefficients, formed once per launch, differ: a face with exactly one end inside
 * the grid carries theta of that end on a ghost-ring side and 0.0 on a zero-flux side; nodes outside the grid stay
 * fixed at 0.  One sweep, every operation rounded once in this order (no contraction), from the previous sweep's u:
 *     once per node:  g = f / inv_h2
 *                     w = omega / ((cE + cW) + (cS + cN))            a missing face enters as the coefficient 0.0
 *     per sweep:      a  = (cE*(uE - u) + cW*(uW - u)) + (cS*(uS - u) + cN*(uN - u))
 *                     u' = u + w * (a - g)
 * a is the face sum of srpde_div_apply_bc in its order: the missing face is a coefficient 0 in its place, not a
 * skipped term, so its product 0 * (0 - u) = -+0 is added like any other.  A host restatement in that order reproduces
 * the result bit for bit, whatever the tiling or the launch split; bc = 0 runs srpde_div_relax's kernels and gives its
 * bits.  The error operator is I - omega diag(-D)^-1 (-D) with D the operator with the sides bc: -D is still a
 * symmetric, weakly diagonally dominant M-matrix (singular for bc = 15, where the constants are a fixed point of
 * every sweep with f = 0), so for 0 < omega <= 1 no error component grows, and bc = 15 is allowed: a sweep never
 * inverts D.  Refused: bc outside 0 .. 15; bc != 0 with interior_only != 0 (the ring is held and no ghost face is ever
 * read); bc != 0 with n < 2 (a lone node with both faces of an axis missing can have cE + cW + cS + cN = 0).  The
 * workspace is srpde_div_relax_workspace_size's; every other rule is srpde_div_relax's. */
int srpde_div_relax_bc(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                       int face_mean, int bc, double inv_h2, int sweeps, double omega, int interior_only,
                       void* workspace, size_t ws_bytes, hipStream_t stream);
/* srpde_physics_loss_div_fwd with the sides bc on the kind-0 (whole-domain) samples (ABI 23).  There a(y) and the
 * adjoint Dt(m r) are the face sum with the sides bc (coefficient 0 for a missing ghost face, in its place; the
 * operator stays symmetric), and D_theta 1 = -k_d theta with k_d the number of the node's ghost faces on ghost-ring
 * sides only:
 *     r = ((u_std a(y) + u_mean (-k_d theta)) / h^2 - f) / f_std          (fp32, in this split form)
 * With bc = 15, k_d = 0 everywhere and the term does not see u_mean: D_theta 1 = 0.  A kind-1 sample (a crop, interior
 * nodes counted) never reads a ghost face with a non-zero factor: it is computed with bc = 0, bit for bit as
 * srpde_physics_loss_div_fwd computes it.  bc = 0 runs that entry's kernels.  bc outside 0 .. 15 is refused.  LDS,
 * samples per workgroup, the fp64 partials in fixed order, the workspace (srpde_physics_loss_div_workspace_size) and
 * the launches are srpde_physics_loss_div_fwd's; the gradient is scaled by srpde_physics_loss_bwd. */
int srpde_physics_loss_div_fwd_bc(const float* y, const float* t, const float* x, const int* kind, const float* stats,
                                  int B, int n, int face_mean, int bc, float weight, float inv_h2_std,
                                  float inv_h2_sub, float* loss, float* dy_unit, void* workspace, size_t ws_bytes,
                                  hipStream_t stream);

/* ---- Boundary values and prescribed fluxes (ABI 23, extended).  The entries above are homogeneous: a Dirichlet side's ghost
 *      ring holds 0, a zero-flux side's flux is 0.  The entries here take the side mask bc, 0 .. 15 as above (0: four
 *      Dirichlet sides), and boundary data bd, fp64 [Bd][4][n], 8-byte aligned, with bd_stride = 4 n doubles between
 *      problems (Bd = B) or 0 (Bd = 1, one [4][n] for every problem).  The sides are in the mask's order -- row 0,
 *      row n - 1, column 0, column n - 1 -- entry k of a row side belongs to column k, entry k of a column side to
 *      row k; a corner node receives data from both of its sides.
 *          Dirichlet side (bit clear): bd is the value g of the ghost node beyond the edge node a.  The ghost face
 *              keeps its coefficient theta_a and contributes theta_a * (g - u_a) to the face sum: the term of the
 *              entries above with g in place of 0.
 *          flux side (bit set): bd is the outward flux q = theta du/dn through the face half a cell beyond the edge
 *              node.  The ghost face keeps the coefficient 0; the node's divergence gains q / h.
 *      A_bd u, every operation rounded once in this order (no contraction):
 *          1. the face sum of srpde_div_apply_bc on halo tiles whose out-of-grid entries beyond Dirichlet sides hold g
 *             (beyond flux sides and in the halo's corners they hold 0 as before);
 *          2. * inv_h2;
 *          3. only at a node with at least one flux-side ghost face: + ((qE + qW) + (qS + qN)) * inv_h, an absent term
 *             0.0, inv_h = sqrt(inv_h2) formed once on the host;
 *          4. - sigma * u as srpde_div_apply_shift (sigma = 0: the unshifted kernel).
 *      So A_bd u = D_bc u - sigma u + b(bd, theta) with b = A_bd 0 at sigma = 0, non-zero on edge nodes only: an affine
 *      extension.  (D_bc - sigma I) u = f - b is the problem solved; the iteration, the preconditioner, the bound
 *      cond <= theta_max / theta_min and the adjoint solve are the homogeneous ones.  bd = 0 gives the numbers of the
 *      *_bc namesakes (a zero may differ in sign).  The data is read for out-of-grid halo entries and edge nodes only.
 *      Every kernel is one launch on the namesake's tiles: vector stores, no atomics, no grid barrier, no scratch.
 *      bc = 15 with sigma = 0 stays singular and refused; the compatibility of its data is the caller's business. ---- */
/* y = A_bd u: srpde_div_apply_bc's arguments and launch plus the data; y must not alias u, theta or bd. */
int srpde_div_apply_bd(const double* u, const double* theta, double* y, int B, int n, int face_mean, double inv_h2,
                       double sigma, int bc, const double* bd, long long bd_stride, hipStream_t stream);
/* srpde_div_step_rhs_bc with A_bd u (sigma = 0, inv_h2 = (n - 1)^2, inv_h = n - 1) in place of D_theta u in
 * Crank-Nicolson's right-hand side, for data constant in time: rhs = (2 f - sigma * u) - A_bd u.  Backward Euler reads
 * no neighbour: its launch and bits are srpde_div_step_rhs's. */
int srpde_div_step_rhs_bd(const double* u, const double* f, const double* theta, double* rhs, int B, int n,
                          int face_mean, double sigma, int cn, int bc, const double* bd, long long bd_stride,
                          hipStream_t stream);
/* The start of the CG for A_bd u = f, i.e. (D_bc - sigma I) u = f - b: x = u0 (u0 == NULL: zeros, the bits of a zero
 * field), r = f - A_bd u0 in one fused pass, z = M^-1 r, then srpde_div_cg_init_from's k = 0 pass at the real rtol.
 * The stop rule's reference norm is |f - b|: per node b = (ghost faces' terms theta_a * g, summed (E + W) + (S + N),
 * 0.0 for a face to a grid node) * inv_h2, then + ((qE + qW) + (qS + qN)) * inv_h on a flux-side node, then the one
 * subtraction f - b; its square is summed in the same pass with srpde_div_cg_init_from's partials for |f|^2 (per-block
 * partials, fixed order).  resid becomes |r| / |f - b|, and |f - b| = 0 returns u = 0, which then is the solution.  So
 * Laplace's equation, f = 0 with g != 0, iterates: |f| alone would stop it at u = 0 after no iteration.
 * bc = 0 takes the sine-transform plan and a workspace of srpde_div_cg_workspace_size -- all-Dirichlet data keeps the
 * one-launch transform at small n -- and is followed by srpde_div_cg_iterate(_shift); bc != 0 takes the separable plan
 * for bc and srpde_div_cg_workspace_size_bc, followed by srpde_div_cg_iterate_bc.  Those and srpde_div_cg_finish run
 * unchanged: the iteration is homogeneous. */
int srpde_div_cg_init_from_bd(const double* f, const double* u0, const double* theta, int B, int n, int face_mean,
                              int bc, double sigma, double sigma_p, double rtol, const double* bd, long long bd_stride,
                              const void* plan, size_t plan_bytes, void* ws, size_t ws_bytes, hipStream_t stream);
/* srpde_div_theta_grad_bc with g in u's out-of-grid halo beyond Dirichlet sides and 0 in lam's: such a ghost face gives
 * (1 * (g - u_a)) * (0 - lam_a).  The prescribed flux does not depend on theta. */
int srpde_div_theta_grad_bd(const double* u, const double* lam, const double* theta, double* g_out, int B, int n,
                            int face_mean, double inv_h2, double scale, int bc, const double* bd, long long bd_stride,
                            hipStream_t stream);
/* out [B][4][n] = d<lam, A_bd u>/d bd, with a the side's edge node of entry k: (inv_h2 * theta_a) * lam_a on a Dirichlet
 * side, inv_h * lam_a (inv_h = sqrt(inv_h2)) on a flux side.  It depends on neither u nor the face mean.  One
 * edge-gather launch; out must not alias lam or theta.  A caller with Bd = 1 sums out over the batch. */
int srpde_div_bd_grad(const double* lam, const double* theta, double* out, int B, int n, double inv_h2, int bc,
                      hipStream_t stream);
/* srpde_div_relax_bc with boundary data (no interior_only; n >= 2; bc = 0: four Dirichlet sides with values).  An
 * out-of-grid position straight beyond a Dirichlet side's edge node holds g and stays fixed at it through every sweep;
 * a node on a flux side forms, once per launch,
 *     g = (f - ((qE + qW) + (qS + qN)) * inv_h) / inv_h2                 (every other node: g = f / inv_h2)
 * and the sweep is srpde_div_relax_bc's, untouched: a fixed point satisfies A_bd u = f.  Bit-equal to one plain host
 * pass per sweep in this order, whatever the tiling and the launch split. */
int srpde_div_relax_bd(const double* u_in, const double* f, const double* theta, double* u_out, int E, int n,
                       int face_mean, int bc, double inv_h2, int sweeps, double omega, const double* bd,
                       long long bd_stride, void* workspace, size_t ws_bytes, hipStream_t stream);
/* srpde_physics_loss_div_fwd_bc with boundary data on the kind-0 (whole-domain) samples (ABI 23, extended).  bd is
 * FP32 here, [Bd][4][n] in RAW units (not normalised), 4-byte aligned, the sides and the meaning of an entry as above: g
 * at the ghost node beyond a Dirichlet side of bc, the outward flux q through a flux side; bd_stride = 4 n floats
 * between samples or 0 for one [4][n] shared by all (anything else is refused).  The kind-0 residual keeps the split
 * form and gains the affine term b of srpde_div_apply_bd:
 *     r = ((u_std a(y) + u_mean (-k_d theta) + beta) / h^2 + Q inv_h - f) / f_std
 * beta = (tE + tW) + (tS + tN), a term theta_a * g for a ghost face on a Dirichlet side and 0.0 for every other face;
 * Q = (qE + qW) + (qS + qN), an absent term 0.0, only at nodes with a flux-side ghost face; inv_h = sqrt(inv_h2_std),
 * formed once on the host in fp64 and rounded to fp32.  A corner node takes data from both of its sides.  The order of
 * the fp32 operations, each rounded once unless the compiler contracts a product into the sum that follows it:
 *     1. lap = fma(u_std, a(y), u_mean * (-k_d theta)), as srpde_physics_loss_div_fwd_bc;
 *     2. at an edge node: lap + beta;
 *     3. num = lap * inv_h2_std - f, the expression of srpde_physics_loss_div_fwd_bc;
 *     4. at a node with a flux-side ghost face: num + Q * inv_h;
 *     5. r = num / f_std.
 * (f is subtracted before the flux term is added, so that zero data gives the numbers of the _bc entry; a zero may
 * differ in sign.)  b does not depend on y: the gradient is the _bc entry's Dt(m r) with this r, scaled by
 * srpde_physics_loss_bwd.  A kind-1 sample is computed bit for bit as by srpde_physics_loss_div_fwd; its rows of bd are
 * never read, whatever they hold.  The kernel is the _bc entry's with the kind-0 samples' data staged once into LDS
 * (4 n floats per sample behind the three tiles, 52 KiB at n = 64): the same tiles, samples per workgroup, fp64
 * partials in fixed order, workspace (srpde_physics_loss_div_workspace_size) and two launches; no atomics, no scratch.
 * bd == NULL runs srpde_physics_loss_div_fwd_bc. */
int srpde_physics_loss_div_fwd_bd(const float* y, const float* t, const float* x, const int* kind, const float* stats,
                                  int B, int n, int face_mean, int bc, float weight, float inv_h2_std,
                                  float inv_h2_sub, const float* bd, long long bd_stride, float* loss, float* dy_unit,
                                  void* workspace, size_t ws_bytes, hipStream_t stream);

/* ---- Face fluxes and wall totals of the divergence-form operator (ABI 23, extended).  The grid, face_mean, the side
 *      mask bc (0 .. 15) and bd / bd_stride are those of the *_bd entries, except that bd may be NULL here: g = 0 beyond
 *      every Dirichlet side and q = 0 through every flux side.  inv_h = sqrt(inv_h2) and h = 1 / inv_h are formed once
 *      on the host.  Nothing is refused for bc = 15: no solve is involved.
 *      The fields are theta du/dx and theta du/dy on the faces, fp64:
 *          Fx [B][n][n + 1]: entry (i, j) is the face between nodes (i, j - 1) and (i, j); j = 0 and j = n are the wall
 *                            faces of column 0 and column n - 1.
 *          Fy [B][n + 1][n]: entry (i, j) is the face between nodes (i - 1, j) and (i, j); i = 0 and i = n are the wall
 *                            faces of row 0 and row n - 1.
 *      Every operation is rounded once in the order written (no contraction):
 *          a face between two nodes:       F = (c * (u_hi - u_lo)) * inv_h,  c = face_mean(theta_lo, theta_hi) as above;
 *          a wall face, Dirichlet side:    c = theta_a of the edge node a and the ghost value is g:
 *                                          low wall (theta_a * (u_a - g)) * inv_h, high wall (theta_a * (g - u_a)) * inv_h;
 *          a wall face, flux side:         low wall -q, high wall +q, copied (q is the OUTWARD flux theta du/dn, and the
 *                                          low walls' outward normal is -x / -y).
 *      In exact arithmetic ((Fx[i][j+1] - Fx[i][j]) + (Fy[i+1][j] - Fy[i][j])) * inv_h is srpde_div_apply_bd at sigma = 0.
 *      The wall totals are W [B][4], the sides in the mask's order: W_s = h * (the sum over the side's n wall faces of
 *      the outward flux -Fy[0][k], +Fy[n][k], -Fx[k][0], +Fx[k][n]), the integral of theta du/dn over the wall.  A
 *      Dirichlet side's term is (theta_a * (g - u_a)) * inv_h -- the bits of the face flux, its sign turned on a low
 *      wall -- and a flux side's is q.  The sum is in fp64 in one fixed order that depends on n alone: thread t of 256
 *      adds entries t, t + 256, ... in turn, then the 64 lanes of a wave by the xor butterfly and the four waves as
 *      (0 + 1) + (2 + 3); then one product with h.  So W of a problem does not depend on B or on its place in the
 *      batch, and sum_s W_s = h^2 * sum_a (A_bd u)_a at sigma = 0 in exact arithmetic: the discrete divergence theorem.
 *      No atomics, no scratch; every pointer 8-byte aligned; no output may alias an input. ---- */
/* Fx and Fy in one launch on srpde_div_apply_bd's 64 x 32 halo tiles: every node writes its low-x and its low-y face,
 * the nodes of column n - 1 and of row n - 1 the high wall face too, so each face is written once. */
int srpde_div_face_flux(const double* u, const double* theta, double* Fx, double* Fy, int B, int n, int face_mean,
                        double inv_h2, int bc, const double* bd, long long bd_stride, hipStream_t stream);
/* The adjoint of srpde_div_face_flux in u and theta, one gather launch: node a collects from its four faces
 * gW = gFx[i][j], gE = gFx[i][j + 1], gN = gFy[i][j], gS = gFy[i + 1][j]:
 *     gu_a     = ((cW * gW - cE * gE) + (cN * gN - cS * gS)) * inv_h
 *     gtheta_a = (((dW * (u_a - u_W)) * gW + (dE * (u_E - u_a)) * gE)
 *                + ((dN * (u_a - u_N)) * gN + (dS * (u_S - u_a)) * gS)) * inv_h
 * with c the face coefficient and d its derivative in theta_a as in srpde_div_theta_grad_bd: theta_a and 1 towards a
 * Dirichlet ghost face (u there is g), 0 towards a flux side's wall face, whose flux is data.  gu or gtheta may be NULL.
 * The gradient in bd touches wall faces only: -+ theta_a * inv_h * gF on a Dirichlet side's low / high wall, -+ gF on
 * a flux side's, which a caller forms from the edge rows. */
int srpde_div_face_flux_grad(const double* u, const double* theta, const double* gFx, const double* gFy, double* gu,
                             double* gtheta, int B, int n, int face_mean, double inv_h2, int bc, const double* bd,
                             long long bd_stride, hipStream_t stream);
/* W [B][4]: an edge gather and the fixed-order sum above, one workgroup per side and problem; reads the 4 n edge nodes
 * of a problem, never its interior.  face_mean is checked and unused: a wall face has c = theta_a. */
int srpde_div_wall_flux(const double* u, const double* theta, double* W, int B, int n, int face_mean, double inv_h2,
                        int bc, const double* bd, long long bd_stride, hipStream_t stream);
/* The adjoint of srpde_div_wall_flux, three [B][4][n] outputs (any may be NULL) in one edge-gather launch like
 * srpde_div_bd_grad's.  With w = gW[b][s] * h and a the edge node of entry k of side s:
 *     Dirichlet side:  gu_edge = -((theta_a * inv_h) * w),  gtheta_edge = ((g - u_a) * inv_h) * w,
 *                      gbd = (theta_a * inv_h) * w
 *     flux side:       gu_edge = 0, gtheta_edge = 0, gbd = w
 * The caller adds the four edge rows into zero fields (a corner node receives from both of its sides) and sums gbd
 * over the batch for shared data. */
int srpde_div_wall_flux_grad(const double* gW, const double* u, const double* theta, double* gu_edge,
                             double* gtheta_edge, double* gbd, int B, int n, double inv_h2, int bc, const double* bd,
                             long long bd_stride, hipStream_t stream);

/* ---- Row-sharded CG for ONE n x n problem over `world` ranks (the 640^2 ground
 *      truth of solve_multi_resolution, src/resolution_comparison.py:62-73).  Rank `rank` owns the
 *      rows [row0, row0 + nloc) (rank order tiles [0, n)); f / theta / u are its [nloc][n] fp64
 *      rows.  Per iteration k the caller runs
 *        iter_a(k) -> all-gather spq (1 double per rank) into gpq[world]
 *        iter_b(k) -> all-gather send (4n + 1 doubles per rank) into gath[world][4n + 1]
 *      after init (whose send buffer is gathered first); gath / gpq may alias send / spq at world 1.
 *      Convergence (rr <= rtol^2 rr_0 or k = maxit) is decided identically on every rank; the int
 *      at byte srpde_poisson_rows_done_offset of the workspace turns nonzero then (poll it every few
 *      dozen iterations; further calls are no-ops).  No call synchronises the host. */
size_t srpde_poisson_rows_workspace_size(int n, int nloc);
size_t srpde_poisson_rows_done_offset(int n, int nloc);
int srpde_poisson_rows_init(const double* f, const double* theta, int n, int nloc, void* ws, size_t ws_bytes,
                            double* send, hipStream_t stream);
int srpde_poisson_rows_iter_a(int n, int nloc, int row0, int rank, int world, const double* gath, int k, int maxit,
                              double rtol, void* ws, size_t ws_bytes, double* spq, hipStream_t stream);
int srpde_poisson_rows_iter_b(int n, int nloc, int world, const double* gath, const double* gpq, int k, void* ws,
                              size_t ws_bytes, double* send, hipStream_t stream);
int srpde_poisson_rows_finish(double* u, int* iters, int n, int nloc, int maxit, void* ws, size_t ws_bytes,
                              hipStream_t stream);

/* ---- Streamed training samples (online.SampleStream): the random draws of the reference's dataset generators
 *      (np.random.uniform / randint per sample, src/data_generation.py:130-131, src/enhanced_data_generation.py:
 *      123-138) from a counter-based generator on the device, and the crop / stride / fp32 cast of
 *      generate_subdomain_dataset + PDEDataset (enhanced_data_generation.py:141-148, src/models.py:132-203) as one
 *      pass.  The generator is Philox4x32-10, a pure function of (seed, sample, field, element):
 *          key = (seed low word, seed high word), counter = (element, field, sample low word, sample high word)
 *      so a sample's values depend on nothing else -- not on B, the rank count or the launch geometry.  An
 *      ordered pair of output words (a, b) gives the double u = (((uint64)a << 32 | b) >> 11) * 2^-53 in [0, 1).
 *          field 0, element 0: k1 from words 0,1 and k2 from words 2,3
 *          field 0, element 1: start_x from words 0,1 and start_y from words 2,3
 *          field 1, element e: theta pixels 2e (words 0,1) and 2e + 1 (words 2,3) of the row-major [n][n] grid
 *          field 2, element e = 0 .. 7: side e >> 1 of the boundary data (srpde_stream_walls), cosine modes
 *                              m = 2 (e & 1) from words 0,1 and m + 1 from words 2,3
 *      A value in [lo, hi) is lo + (hi - lo) * u (a rounded product, then a rounded sum), a start is
 *      (int)floor(u * max_start), so 0 <= start < max_start as np.random.randint(0, max_start).  All entries are
 *      stream-ordered, keep no state and never synchronise the host. ---- */
/* The raw words: out[(s * n_elements + e) * 4 + w] = word w of (seed, sample0 + s, field, element0 + e), for
 * n_samples x n_elements <= 2^31 counters; field and element0 + n_elements - 1 fit 32 bits, sample0 + s wraps in
 * 64 bits.  (The known-answer hook: any Philox4x32-10 counter / key can be asked for.) */
int srpde_stream_raw(long long seed, long long sample0, long long n_samples, long long field, long long element0,
                     long long n_elements, unsigned* out, hipStream_t stream);
/* The draws of samples sample0 .. sample0 + B - 1 in one launch: k12 [B][2] fp64 in [k_lo, k_hi); starts [B][2]
 * int32 (x, y) in [0, max_start) (nullable: no starts drawn, max_start ignored); theta [B][n][n] fp64 (nullable:
 * n ignored), with theta_mode 0 exactly 1.0 everywhere and with theta_mode 1 uniform in [theta_lo, theta_hi);
 * theta_half (nullable) [B][(n + 1) / 2][(n + 1) / 2] = theta[:, ::2, ::2], the coefficient of a coarse solve. */
int srpde_stream_draw(long long seed, long long sample0, int B, double k_lo, double k_hi, int theta_mode,
                      double theta_lo, double theta_hi, int n, int max_start, double* k12, int* starts, double* theta,
                      double* theta_half, hipStream_t stream);
/* From the solved fields u, f, theta [B][ns][ns] fp64 and starts [B][2] int32 (x, y) on the device: the fp32 training
 * fields u_fine, f_fine, theta_fine [B][nf][nf] = field[start_y + i][start_x + j] and u_coarse [B][nc][nc],
 * nc = (nf + 1) / 2, the stride-2 subsample of the u window -- extract_subdomain + downsample + the fp32 cast.  A
 * start outside [0, ns - nf] is clamped into it.  starts == NULL is the pass-through for standard samples: ns == nf,
 * the window at (0, 0), and u_coarse is the fp32 cast of u_coarse_in [B][nc][nc], the sample's own coarse solve
 * (u_coarse_in == NULL: the subsample, as above; u_coarse_in with starts is refused). */
int srpde_stream_window(const double* u, const double* f, const double* theta, const int* starts,
                        const double* u_coarse_in, int B, int ns, int nf, float* u_fine, float* f_fine,
                        float* theta_fine, float* u_coarse, hipStream_t stream);
/* Smooth random boundary data for samples sample0 .. sample0 + B - 1 on a side of n nodes (ABI 23, extended), the
 * layout of the *_bd entries: bd [B][4][n] fp64, the sides in the order of the mask bc (0 .. 15).  Side s has four
 * coefficients from field 2: c_m = (amp * (2 u - 1)) / (m + 1), m = 0 .. 3, with u the [0, 1) double above (2 u - 1 is
 * exact; the product, then the quotient, rounded once each) and amp = g_amp on a Dirichlet side (bit clear: the entries
 * are ghost values), q_amp on a flux side (bit set: outward fluxes).  Then, every operation rounded once (no contraction),
 *     bd[b][s][k] = (c0 cos(0) + c1 cos(pi k / (n - 1))) + (c2 cos(2 pi k / (n - 1)) + c3 cos(3 pi k / (n - 1)))
 * with the argument reduced in integers, cos(pi m k / (n - 1)) = cospi(((m k) mod 2 (n - 1)) / (n - 1)).  So |bd| <=
 * (25 / 12) amp.  bd_half (nullable) [B][4][(n + 1) / 2] = bd[..., ::2], the data of the stride-2 coarse solve;
 * bd_f32 (nullable) [B][4][n] is the fp32 cast of bd, what srpde_physics_loss_div_fwd_bd reads.  One launch, a pure
 * function of (seed, sample, bc, g_amp, q_amp, n); n >= 2, finite amplitudes. */
int srpde_stream_walls(long long seed, long long sample0, int B, int n, int bc, double g_amp, double q_amp, double* bd,
                       double* bd_half, float* bd_f32, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SRPDE_H_ */
