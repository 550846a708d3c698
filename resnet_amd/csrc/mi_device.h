/*
 * mi_device.h -- the thin header layer between the C host code (trainer.c, loader.c, ...) and the
 * HIP side (runtime.hip + kernels_*.hip).  Host .c files include only this; they never see HIP
 * headers.  It plays the role of the cuda_runtime.h include of resnet.cu:5-7 plus the
 * prepareAndDo* launch wrappers of resnet.cu:1386-1509.
 * All launches are asynchronous on the given stream; errors are recorded (mid_last_error).
 */
#ifndef MI_DEVICE_H
#define MI_DEVICE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void *mid_stream;
typedef void *mid_event;

/* storage type of an activation tensor (parameters, gradients and statistics are always fp32) */
enum { MID_F32 = 0, MID_BF16 = 1 };

/* ---- runtime ---- */
int mid_device_count(void);
int mid_set_device(int dev);
const char *mid_last_error(void);
void mid_clear_error(void);
void *mid_malloc(size_t bytes);
void mid_free(void *p);
/* red-zone mode of mid_malloc / mid_free (test aid, runtime.hip): zone | payload | zone, all filled with fill_byte, zones compared at free and in
 * mid_redzone_check */
int mid_redzone(size_t zone_bytes, int fill_byte);
int mid_redzone_check(void);
void mid_redzone_stats(size_t *allocs_checked, size_t *zone_bytes_checked, size_t *live);
/* the launch ring of RESNET_MI_TRACE=1 (runtime.hip): its names oldest first, one per line, into buf; returns how many it holds */
int mid_trace_names(char *buf, size_t cap);
void mid_trace_clear(void);
void *mid_malloc_host(size_t bytes); /* pinned */
void mid_free_host(void *p);
void mid_memcpy_h2d(void *dst, const void *src, size_t bytes, mid_stream s);
void mid_memcpy_d2h(void *dst, const void *src, size_t bytes, mid_stream s);
void mid_memcpy_d2d(void *dst, const void *src, size_t bytes, mid_stream s);
void mid_memset(void *dst, int byte, size_t bytes, mid_stream s);
mid_stream mid_stream_create(void);
mid_stream mid_stream_create_low_priority(void);
void mid_stream_destroy(mid_stream s);
void mid_stream_sync(mid_stream s);
void mid_device_sync(void);
mid_event mid_event_create(void);
void mid_event_destroy(mid_event e);
void mid_event_record(mid_event e, mid_stream s);
void mid_stream_wait_event(mid_stream s, mid_event e);
float mid_event_elapsed_ms(mid_event a, mid_event b);
void mid_event_sync(mid_event e);

/* ---- optional per-kernel-family timing (HIP events around each launch, on the launch stream) ----
 * families: 0 direct conv fwd/dgrad, 1 direct conv wgrad, 2 MFMA GEMM (1x1 conv, FC), 3 batch norm, 4 other */
void mid_prof_enable(int on);
void mid_prof_reset(void);
/* resolves pending events (synchronises) and returns totals since the last reset */
void mid_prof_get(int family, long *launches, double *ms, double *flops, double *bytes);

/* ---- workspace a conv launch may use (transformed weights, split partials) ---- */
typedef struct {
    float *wt;        /* transformed-weight scratch */
    size_t wt_floats;
    float *part;      /* split-reduction partial sums */
    size_t part_floats;
    /* weights of the NEXT call already re-laid by mid_conv_prelayout_all (else NULL: the call re-lays them itself into wt) */
    const float *pre_fwd, *pre_dgrad;
    /* bf16 path, stride-2 layers: scratch for x re-laid as four parity planes per channel (>= 2 bytes per element of x, with the
     * guard bytes of every bf16 tensor on both sides); NULL = those layers gather element-wise */
    void *s2d;
    size_t s2d_bytes;
    int s2d_valid; /* s2d already holds the parity planes of this call's x (the forward pass of the same layer wrote them) */
} mid_workspace;

/* One launch that re-lays the weights of many convolutions for the implicit-GEMM kernel: fwd = [t][c][k], dgrad = [t][k][c]
 * (either may be NULL).  entries / tile_entry live in device memory; tile0 = first 32x32 (k, c) tile of the entry in the
 * launch's flat tile numbering, tile_entry[tile] = its entry. */
typedef struct {
    const float *w;
    float *fwd, *dgrad;
    int K, C, T, tile0;
} mid_wt_entry;
int mid_conv_prelayout_all(mid_stream s, const mid_wt_entry *entries_dev, const int *tile_entry_dev, int ntiles);

/* ---- convolution (NCHW activations, KCRS weights), square images/kernels, pad k/2, Ho = H/stride ---- */
/* The fp32 kernels, one launcher each.  Which of them a convolution runs is named once, by the planner (layer.c, MI_K_*): nothing here
 * chooses.  Every launcher returns 0, or < 0 with the error recorded where it is handed a shape its kernel does not take (-2) or a
 * workspace smaller than its size function asks for (-3). */
/* Batch-norm statistics fused into the producing convolution: the implicit-GEMM kernel (and the bf16, channel-last and stem
 * kernels) has every workgroup also write per-channel (count, mean, M2) partials of its output tile into parts->buf (three planes of
 * [nparts][K]); parts->nparts comes back > 0.  0 = not fused: run the separate statistics pass (mid_bn_fwd). */
typedef struct {
    float *buf;
    size_t floats;
    int nparts;
} mid_bn_parts;
size_t mid_bn_parts_floats(int N, int K, int Ho);
/* The REDUCTION pass of a batch-norm backward fused into the dgrad that produces its dy (bf16 kernels, pixel-major epilogue; fp32
 * implicit GEMM at stride 1): the dgrad stores g = (mask > 0 ? dx : 0) instead of dx and leaves per-tile sums of g and g (x - mean) per
 * channel in buf (two planes [nparts][C]); nparts comes back > 0 when the launch could do it.  mid_bn_bwd_parts_t then finishes that
 * batch norm (merge, finalize, apply) without reading dy for the sums. */
typedef struct {
    const void *x;       /* the BN's input (the convolution output it normalised), the shape of the dgrad output */
    const void *mask;    /* the tensor whose sign gates: that BN's activated output, or the block output for the expansion BN */
    const float *means;
    float *buf;
    size_t floats;
    int nparts;
} mid_bn_bwd_parts;
/* igemm_kernel (kernels_igemm.hip): MFMA implicit GEMM for the 3x3 / 1x1 shapes that tile.  mi_igemm_supported: its shape and size gate
 * (op 0 fwd, 1 dgrad, 2 wgrad); the workspace holds the re-laid weights (mid_conv_ws_wt_floats; with mi_igemm_tail_floats more behind
 * them, the partial tiles of the reduction-sliced tail workgroups, compute stream only) and the weight gradient's split partials.
 * dx = dgrad (+ addend when addend != NULL; addend may alias dx); fz (optional, stride 1): see mid_bn_bwd_parts */
int mi_igemm_supported(int op, int N, int C, int H, int K, int k, int stride);
size_t mi_igemm_tail_floats(void);
size_t mi_igemm_part_floats(int N, int C, int H, int K, int k, int stride);
int mi_igemm_fwd(mid_stream s, mid_workspace *ws, const float *x, const float *w, float *y, int N, int C, int H, int K, int k, int stride,
                 mid_bn_parts *parts);
int mi_igemm_dgrad(mid_stream s, mid_workspace *ws, const float *w, const float *dy, float *dx, const float *addend, int N, int C, int H,
                   int K, int k, int stride, mid_bn_bwd_parts *fz);
int mi_igemm_wgrad(mid_stream s, mid_workspace *ws, const float *x, const float *dy, float *dw, int N, int C, int H, int K, int k, int stride);
/* gemm_mfma_kernel (kernels_gemm.hip): a 1x1 stride-1 convolution over P = H * H pixels as a plain MFMA GEMM, any channel counts */
int mi_conv1x1_fwd(mid_stream s, const float *x, const float *w, float *y, int N, int C, int P, int K);
int mi_conv1x1_dgrad(mid_stream s, const float *w, const float *dy, float *dx, const float *addend, int N, int C, int P, int K);
size_t mi_conv1x1_wgrad_part_floats(int N, int C, int P, int K);
int mi_conv1x1_wgrad(mid_stream s, mid_workspace *ws, const float *x, const float *dy, float *dw, int N, int C, int P, int K);
/* dconv_kernel, wgradC_kernel, wgrad_kernel (kernels_conv.hip): direct LDS-tiled VALU kernels -- forward 3x3 (stride 1 / 2) and the 7x7
 * stem, dgrad 3x3, weight gradient in the C form (3x3, C % 64 == 0, K % 32 == 0, planes its chunks tile) or the read-lane form
 * (3x3 and 7x7, K % 64 == 0).  The workspace holds the re-laid weights (mid_conv_ws_wt_floats) and the weight gradient's partials */
size_t mid_conv_ws_wt_floats(int C, int K, int k);
int mid_direct_fwd(mid_stream s, mid_workspace *ws, const float *x, const float *w, float *y, int N, int C, int H, int K, int k, int stride);
int mid_direct_dgrad(mid_stream s, mid_workspace *ws, const float *w, const float *dy, float *dx, const float *addend, int N, int C, int H,
                     int K, int k, int stride);
int mid_direct_wgradC_supported(int N, int C, int H, int K, int k, int stride);
size_t mid_direct_wgradC_part_floats(int N, int C, int H, int K, int k, int stride);
int mid_direct_wgradC(mid_stream s, mid_workspace *ws, const float *x, const float *dy, float *dw, int N, int C, int H, int K, int k, int stride);
size_t mid_direct_wgrad_part_floats(int N, int C, int H, int K, int k, int stride);
int mid_direct_wgrad(mid_stream s, mid_workspace *ws, const float *x, const float *dy, float *dw, int N, int C, int H, int K, int k, int stride);

/* ---- bf16-activation path (kernels_igemm_bf16.hip): x / y / dy / dx are bf16 NCHW, weights fp32 KCRS (rounded to bf16 when
 * re-laid), weight gradients fp32.  ws->pre_fwd / pre_dgrad point at bf16 k-step tiles when mid_conv_prelayout_all_bf16 made
 * them; otherwise the call re-lays the weights itself into ws->wt. ---- */
int mid_bf16_supported(int op, int N, int C, int H, int K, int k, int stride); /* op 0 fwd, 1 dgrad, 2 wgrad */
int mid_conv_prelayout_all_bf16(mid_stream s, const mid_wt_entry *entries_dev, const int *tile_entry_dev, int ntiles);
int mid_conv_fwd_bf16(mid_stream s, mid_workspace *ws, const void *x, const float *w, void *y, int N, int C, int H, int K, int k,
                      int stride, mid_bn_parts *parts);
int mid_conv_dgrad_bn_bf16(mid_stream s, mid_workspace *ws, const float *w, const void *dy, void *dx, const void *addend, int N, int C,
                           int H, int K, int k, int stride, mid_bn_bwd_parts *fz);
int mid_bn_bwd_parts_t(mid_stream s, float *stats_ws, const mid_bn_bwd_parts *parts, const void *x, int x_dt, const float *gamma,
                       const float *beta, const float *means, const float *vars, const void *dy_gated, int a_dt, void *dx, float *dgamma,
                       float *dbeta, int N, int C, int P, float eps);
int mid_conv_dgrad_bf16(mid_stream s, mid_workspace *ws, const float *w, const void *dy, void *dx, const void *addend, int N, int C,
                        int H, int K, int k, int stride);
/* bgemm_kernel's weight gradient and its split partials; a 1x1 the planner puts on pw_wgrad_kernel runs mid_pw_wgrad instead */
size_t mi_bgemm_part_floats(int N, int C, int H, int K, int k, int stride);
int mi_bgemm_wgrad(mid_stream s, mid_workspace *ws, const void *x, const void *dy, float *dw, int N, int C, int H, int K, int k, int stride);
/* ---- 3x3 convolutions of the bf16 path on channel-last, zero-padded operands (kernels_cl_bf16.hip): both operands global -> LDS by
 * LDS-DMA, no transposes, no masks.  op 0 forward (stride 1 or 2), op 1 dgrad (stride 1) ---- */
int mid_bf16_prelayout_fwd(mid_stream s, const float *w, void *out, int K, int C, int k);
int mid_bf16_prelayout_dgrad(mid_stream s, const float *w, void *out, int K, int C, int k);
int mid_cl_supported(int op, int N, int C, int H, int K, int stride);
size_t mid_cl_operand_bytes(int op, int N, int C, int H, int K, int stride);
/* x (bf16 NCHW, C channels, H x H) -> padded channel-last; parity != 0: the four parity planes of a stride-2 forward.  The halo of xp
 * must be zero: zero the buffer once when it is made (the kernel writes the interior only) */
int mid_cl_relayout(mid_stream s, const void *x, void *xp, int N, int C, int H, int parity);
int mid_cl_fwd(mid_stream s, const void *xp, const void *a_tiles, void *y, int N, int C, int H, int K, int stride, mid_bn_parts *parts);
int mid_cl_dgrad(mid_stream s, const void *dyp, const void *a_tiles, void *dx, const void *addend, int N, int C, int H, int K);
/* weight gradient from dY (NCHW) and the forward's re-laid input: transposed LDS reads on the pixel-major operand */
int mid_cl_wgrad_supported(int N, int C, int H, int K, int stride);
size_t mid_cl_wgrad_part_floats(int N, int C, int H, int K, int stride);
int mid_cl_pw_supported(int N, int C, int H, int K);
int mid_cl_relayout_dense(mid_stream s, const void *x, void *xp, int N, int C, int H);
int mid_cl_pw_fwd(mid_stream s, const void *xc, const void *a_tiles, void *y, int N, int C, int H, int K, mid_bn_parts *parts);
int mid_cl_wgrad2_supported(int N, int C, int H, int K, int stride);
size_t mid_cl_wgrad2_part_floats(int N, int C, int H, int K, int stride);
int mid_cl_wgrad2(mid_stream s, const void *xp, const void *dyp, float *dw, float *part, size_t part_floats, int N, int C, int H, int K, int stride);
int mid_pw_wgrad_supported(int N, int C, int H, int K);
size_t mid_pw_wgrad_part_floats(int N, int C, int H, int K);
int mid_pw_wgrad(mid_stream s, const void *x, const void *dy, float *dw, float *part, size_t part_floats, int N, int C, int H, int K);
int mid_cl_wgrad(mid_stream s, const void *xp, const void *dy, float *dw, float *part, size_t part_floats, int N, int C, int H, int K, int stride);
/* stride-2 dgrad: dY (K channels, H/2 x H/2) re-laid channel-last with one zero row / column at the far end, both column parities of dx in
 * one workgroup (dense stores) */
int mid_cl_dgrad2_supported(int N, int C, int H, int K);
size_t mid_cl_dgrad2_operand_bytes(int N, int K, int Ho);
int mid_cl_relayout_end(mid_stream s, const void *dy, void *dyp, int N, int K, int Ho);
int mid_cl_dgrad2(mid_stream s, const void *dyp, const void *a_tiles, void *dx, int N, int C, int H, int K);
/* the 7x7 stride-2 stem (3 -> 64 channels) on the bf16 matrix cores (kernels_stem_bf16.hip): image and weights rounded to
 * bf16, fp32 accumulation, fp32 output / output gradient.  xp = the image as zero-padded parity planes (written by the
 * forward, read again by the weight gradient); scratch = wave partials + re-laid weights (mid_stem_bf16_part_floats). */
/* ... and in exact fp32 (v_mfma_f32_32x32x2_f32) for the fp32 storage mode; same shape rule, same scratch, fp32 planes */
size_t mid_stem_f32_xp_bytes(int N, int H);
int mid_stem_fwd_f32(mid_stream s, const float *x, const float *w, float *y, void *xp, size_t xp_bytes, float *scratch, size_t scratch_floats,
                     int N, int H, mid_bn_parts *parts);
int mid_stem_wgrad_f32(mid_stream s, const void *xp, const float *dy, float *dw, float *scratch, size_t scratch_floats, int N, int H);
int mid_stem_bf16_supported(int C, int H, int K, int k, int stride);
size_t mid_stem_bf16_xp_bytes(int N, int H);
size_t mid_stem_bf16_part_floats(int N, int H);
int mid_stem_fwd_bf16(mid_stream s, const float *x, const float *w, void *y, int y_dt, void *xp, size_t xp_bytes, float *scratch, size_t scratch_floats,
                      int N, int H, mid_bn_parts *parts); /* parts (optional): BN statistics partials of y, as mi_igemm_fwd leaves them */
int mid_stem_wgrad_bf16(mid_stream s, const void *xp, const void *dy, int dy_dt, float *dw, float *scratch, size_t scratch_floats, int N, int H);
int mid_f32_to_bf16(mid_stream s, const float *in, void *out, size_t n);
int mid_bf16_to_f32(mid_stream s, const void *in, float *out, size_t n);

/* host-only: route and grid the launch planners choose for a convolution (kernels_igemm.hip); op 0 fwd, 1 dgrad, 2 wgrad */
int mid_igemm_plan(int op, int N, int C, int H, int K, int k, int stride, int out[9]);
/* mi_conv_plan's pieces (resnet_mi.h): the launch planners of the fp32 implicit GEMM, the bf16 NCHW kernels and the channel-last / LDS-DMA
 * kernels; 1 = planned, 0 = the route refuses the shape */
int mid_igemm_conv_plan(int op, int N, int C, int H, int K, int k, int stride, int out[7]);
int mid_bf16_conv_plan(int op, int N, int C, int H, int K, int k, int stride, int out[7]);
int mid_cl_conv_plan(int route, int op, int N, int C, int H, int K, int k, int stride, int out[7]);
int mid_wgrad_reduce_grouped(int K, int C, int splits); /* 1: the split reduce of a weight gradient runs grouped */

/* ---- plain GEMMs for the FC layer (row-major) ---- */
/* out[m x n] = A[m x k] B[k x n] */
int mid_gemm_nn(mid_stream s, const float *A, const float *B, float *out, int m, int k, int n);
/* out[m x n] = At^T B, At is [k x m] */
int mid_gemm_tn(mid_stream s, const float *At, const float *B, float *out, int m, int k, int n);
/* out[m x n] = A Bt^T, Bt is [n x k] */
int mid_gemm_nt(mid_stream s, const float *A, const float *Bt, float *out, int m, int k, int n);

/* ---- batch norm (training mode, biased variance, per-replica statistics) ---- */
/* stats_ws: >= mid_bn_ws_floats(C) floats of scratch */
size_t mid_bn_ws_floats(int C);
/* y = [relu](gamma * (x-mean)/sqrt(var+eps) + beta) [+ residual, relu]; writes means/vars.
 * residual != NULL => y = relu(bn(x) + residual).  xhat_out / norm_out optional (full-store). */
int mid_bn_fwd(mid_stream s, float *stats_ws, const float *x, const float *gamma, const float *beta,
               const float *residual, float *means, float *vars, float *y, float *xhat_out, float *norm_out, int N,
               int C, int P, float eps, int relu);
/* the same with the statistics taken from the partials a convolution left (parts->nparts > 0), else from x */
int mid_bn_fwd_parts(mid_stream s, float *stats_ws, const mid_bn_parts *parts, const float *x, const float *gamma,
                     const float *beta, const float *residual, float *means, float *vars, float *y, float *xhat_out,
                     float *norm_out, int N, int C, int P, float eps, int relu);
/* mask_mode 0 none; 1 recompute own ReLU mask from x; 2 gate dy by mask_src > 0 */
int mid_bn_bwd(mid_stream s, float *stats_ws, const float *x, const float *gamma, const float *beta,
               const float *means, const float *vars, const float *dy, const float *mask_src, float *dx,
               float *dgamma, float *dbeta, int N, int C, int P, float eps, int mask_mode);

/* mask_mode 2 that also writes gated_out = (mask_src > 0 ? dy : 0), the tensor doActivationDeriv (resnet.cu:1934) would
 * have produced in a pass of its own; gated_out may not alias dx */
int mid_bn_bwd_gate(mid_stream s, float *stats_ws, const float *x, const float *gamma, const float *beta,
                    const float *means, const float *vars, const float *dy, const float *mask_src, float *gated_out,
                    float *dx, float *dgamma, float *dbeta, int N, int C, int P, float eps);

/* the same operators over typed tensors: x_dt = storage type of the convolution output x (and of dx), a_dt = of the
 * activation-side tensors (y, residual, dy, mask_src, gated_out).  Pairs: (f32,f32), (bf16,bf16), (f32,bf16).
 * ycl != NULL (mid_bn_fwd_t, mid_bn_apply_t): the (bf16; ReLU or + residual, ReLU) output is also written channel-last for the
 * 3x3 that reads it: Hcl > 0 one plane with a halo of 1, Hcl < 0 the four parity planes of a stride-2 3x3 over |Hcl| x |Hcl|;
 * only the interior is written (the caller zeroes ycl once).  NULL, 0: no side output. */
int mid_bn_fwd_t(mid_stream s, float *stats_ws, const mid_bn_parts *parts, const void *x, int x_dt, const float *gamma,
                 const float *beta, const void *residual, float *means, float *vars, void *y, int a_dt, float *xhat_out,
                 float *norm_out, int N, int C, int P, float eps, int relu, void *ycl, int Hcl);
/* cross-replica batch-norm statistics through `comm` (an RCCL communicator of its own); NULL = per-replica (the reference) */
void mid_bn_set_sync(void *comm, int world, float *tmp, size_t tmp_floats, int force);
/* test aid: the sync-BN merge kernels on R replicas held by one process (the all-reduce replaced by a sum kernel); see kernels_bn.hip */
int mid_bn_debug_merge(mid_stream s, int R, int C, float *means, float *vars, float *dgamma, float *dbeta, float *sums_out, float *tmp);
int mid_bn_stats_t(mid_stream s, float *stats_ws, const void *x, int x_dt, float *means, float *vars, int N, int C, int P);
int mid_bn_apply_t(mid_stream s, const void *x, int x_dt, const float *gamma, const float *beta, const void *residual,
                   const float *means, const float *vars, void *y, int a_dt, int N, int C, int P, float eps, int relu, void *ycl, int Hcl);
/* running statistics (kernels_bn.hip, bn_running_update_kernel): one entry per BN layer -- the layer's batch statistics, its first
 * thread (= the sum of the channel counts before it), its offset into both halves of the running arena, its channels and
 * unbias = n / (n - 1).  One launch updates every layer: rm = (1 - m) rm + m mean, rv = (1 - m) rv + m (var unbias) */
typedef struct { const float *means, *vars; int first, off, C; float unbias; } mid_bn_run_entry;
int mid_bn_running_update(mid_stream s, const mid_bn_run_entry *tab_dev, int n_layers, int channels, float *arena, size_t half, float momentum);
/* mask_mode 0..2 as mid_bn_bwd; 3 = mid_bn_bwd_gate */
int mid_bn_bwd_t(mid_stream s, float *stats_ws, const void *x, int x_dt, const float *gamma, const float *beta, const float *means,
                 const float *vars, const void *dy, const void *mask_src, void *gated_out, int a_dt, void *dx, float *dgamma,
                 float *dbeta, int N, int C, int P, float eps, int mask_mode);
int mid_maxpool_fwd_t(mid_stream s, const void *x, void *y, int dt, int *max_inds, int N, int C, int H, int k, int stride);
int mid_maxpool_bwd_t(mid_stream s, const int *max_inds, const void *dy, void *dx, int dt, int N, int C, int H, int k, int stride);
int mid_avgpool_fwd_t(mid_stream s, const void *x, int dt, float *y, int N, int C, int P);
int mid_avgpool_bwd_t(mid_stream s, const float *dy, void *dx, int dt, int N, int C, int P);

/* ---- pools, elementwise, loss, optimizer ---- */
int mid_maxpool_fwd(mid_stream s, const float *x, float *y, int *max_inds, int N, int C, int H, int k, int stride);
int mid_maxpool_bwd(mid_stream s, const int *max_inds, const float *dy, float *dx, int N, int C, int H, int k,
                    int stride);
int mid_avgpool_fwd(mid_stream s, const float *x, float *y, int N, int C, int P);
int mid_avgpool_bwd(mid_stream s, const float *dy, float *dx, int N, int C, int P);
int mid_relu_deriv(mid_stream s, const float *x, const float *up, float *out, size_t n);
int mid_add_relu(mid_stream s, const float *a, const float *b, float *sum_out, float *act_out, size_t n);
int mid_softmax(mid_stream s, const float *x, float *out, int N, int L);
int mid_ce_deriv(mid_stream s, const float *pred, const int *labels, float *d, int N, int L);
/* the loss head (kernels_loss.hip): soft-max, label-smoothed cross-entropy gradient, per-row loss and rank of the label in one launch;
 * pred / dlogits [N][L], row_loss / row_rank [N], each may be NULL.  With last_dev or total_dev (MiLossMetrics of resnet_mi.h, device
 * memory) a one-wave launch behind it reduces row_loss and row_rank -- both needed then -- into them: last overwritten, total added to */
typedef struct { double loss_sum; int64_t rows, wrong_top1, wrong_topk, batches; } mid_loss_metrics;
int mid_loss_head(mid_stream s, const float *logits, const int *labels, float *pred, float *dlogits, float *row_loss, int *row_rank, int N,
                  int L, float smoothing, int topk, mid_loss_metrics *last_dev, mid_loss_metrics *total_dev);
/* the two-label head of mixup / CutMix: t_j = ((j == a ? wa : 0) + (j == b ? wb : 0)) + u with wa = (1.f - eps) lam, wb = (1.f - eps)
 * (1.f - lam); rank against labels_a; everything else as mid_loss_head, whose bits it gives at lam = 1.f (row_loss apart) */
int mid_loss_head_mix(mid_stream s, const float *logits, const int *labels_a, const int *labels_b, float lam, float *pred, float *dlogits,
                      float *row_loss, int *row_rank, int N, int L, float smoothing, int topk, mid_loss_metrics *last_dev, mid_loss_metrics *total_dev);
/* fused updateMeans+updateVars+updateParams (resnet.cu:605-662).  On NaN/Inf *nan_flag (device int) becomes the highest offending
 * locations[] index + 1 (check_errors, resnet.cu:2879-2907): loc_off_dev = n_loc + 1 arena offsets (floats) of the tensors, base =
 * arena offset of p[0]; loc_off_dev NULL: the flag becomes 1. */
int mid_adam(mid_stream s, float *p, float *g, float *m, float *v, size_t n, float lr, float wd, float b1,
             float b2, float cur_b1, float cur_b2, float eps, int *nan_flag, int zero_grads, const size_t *loc_off_dev, int n_loc,
             size_t base);
/* momentum SGD / LARS (kernels_optim.hip).  The parameter-shaped arenas are cut into chunks of at most MID_OPT_CHUNK floats that
 * never cross a tensor (start: float offset into the arena, a multiple of 4); every pass runs one workgroup per chunk of
 * [c0, c1).  norms: double2 (sum w^2, sum g^2) per chunk into part[2 * chunk].  trust: for tensors [t0, t1) (first_chunk:
 * n_tensors + 1 entries) the partials summed in a fixed order into sq[2 * t] and the LARS trust ratio into trust[t] (NaN: a norm
 * is not finite).  update: the rule of `kind` (MID_OPT_SGD ignores trust and decays the tensors with is_weight 0 by wd_norm, which
 * MID_OPT_LARS ignores); *nan_flag = highest offending tensor + 1 */
enum { MID_OPT_ADAM = 0, MID_OPT_SGD = 1, MID_OPT_LARS = 2 };
#define MID_OPT_CHUNK 8192
typedef struct { int tensor, start, len, pad; } mid_chunk;
int mid_optim_norms(mid_stream s, const float *p, const float *g, const mid_chunk *chunks, int c0, int c1, double *part);
int mid_optim_trust(mid_stream s, const double *part, const int *first_chunk, const int *is_weight, int t0, int t1, float trust_coef,
                    float wd, double *sq, float *trust);
int mid_optim_update(mid_stream s, int kind, float *p, float *g, float *b, const mid_chunk *chunks, int c0, int c1, const int *is_weight,
                     const float *trust, float lr, float wd, float wd_norm, float momentum, int *nan_flag);
/* gradient clipping by the global L2 norm (kernels_optim.hip), over a chunk table of n_chunks chunks that covers the tensors of g and none
 * of the padding between them.  norm: one workgroup per chunk, sum g^2 in double into part[chunk].  coef: one wave sums the partials in a
 * fixed order and writes the record (MiClipRecord of resnet_mi.h, device memory): coef = min(1, max_norm / (sqrt(sq) + 1e-6)) computed in
 * double and rounded to float once; a sum that is not finite gives coef 1 and nonfinite 1; updates goes up by one, clipped where coef < 1.
 * scale: g[i] = g[i] * coef in fp32 where the record's coef is not 1.f -- then no word of g is read or written.  No atomics */
typedef struct { double sq_norm, norm; float coef; int nonfinite; int64_t updates, clipped; } mid_clip_record;
int mid_clip_norm(mid_stream s, const float *g, const mid_chunk *chunks, int n_chunks, double *part);
int mid_clip_coef(mid_stream s, const double *part, int n_chunks, float max_norm, mid_clip_record *rec);
int mid_clip_scale(mid_stream s, float *g, const mid_chunk *chunks, int n_chunks, const mid_clip_record *rec);
/* weight averaging (kernels_optim.hip).  ema[i] = lerp(ema[i], p[i], w), torch.lerp's float32 bits: d = p - e rounded, then fmaf(w, d, e)
 * for w < 0.5f and fmaf(-(1.f - w), d, p) otherwise; a result that is not finite keeps e.  exchange: a[i] <-> b[i] as 32-bit words.  Both
 * pointers 16-byte aligned: 16-byte accesses; otherwise element-wise.  -1, mid_last_error set, nothing launched: a NULL pointer, a pointer
 * that is not 4-byte aligned, w outside [0, 1] or NaN, overlapping ranges (exchange), n == 0 or n > 2^40 */
int mid_ema_update(mid_stream s, float *ema, const float *p, size_t n, float w);
int mid_exchange(mid_stream s, float *a, float *b, size_t n);
void mid_ema_geometry(size_t out[4]); /* [0] threads, floats of one workgroup's turn [1] vector [2] element-wise, [3] the grid's cap */
/* gradient accumulation (kernels_optim.hip), over two arenas of n floats in the geometry of the two above.  FIRST: acc = g as 32-bit words
 * (NaN payloads and -0 as they are); ADD: acc = acc + g; FOLD: g = (acc + g) * scale, sum and product rounded on their own, acc only read.
 * Nothing is guarded: a value that is not finite propagates by IEEE rules.  -1, mid_last_error set, nothing launched: a NULL pointer, a
 * pointer that is not 4-byte aligned, n == 0 or n > 2^40, overlapping ranges, an unknown mode, in FOLD a scale that is NaN, infinite or <= 0 */
enum { MID_ACC_FIRST = 0, MID_ACC_ADD = 1, MID_ACC_FOLD = 2 };
int mid_grad_accumulate(mid_stream s, float *acc, float *g, size_t n, int mode, float scale);
int mid_nhwc_to_nchw(mid_stream s, const float *in, float *out, int N, int H, int W, int C);
int mid_nchw_to_nhwc(mid_stream s, const float *in, float *out, int N, int C, int H, int W);
/* uint8 shards (kernels_input.hip): src = n whole images [dim_in][dim_in][3] bytes (B,G,R interleaved), 16-byte aligned; plan = int [n][3]
 * (row_off, col_off, flip) in device memory; out = fp32 NCHW [n][3][dim_out][dim_out], R,G,B planes, means subtracted as mi_build_shard
 * does.  Reads nothing outside [src, src + n dim_in^2 3).  Returns 0, -1 (alignment / sizes; mid_last_error says which), -2 (dim_out too large) */
int mid_decode_u8(mid_stream s, const uint8_t *src, const int *plan, float *out, int n, int dim_in, int dim_out);
/* boxes [n][5] (row0, col0, h, w, flip), clamped into the image; each box resampled to dim_out^2.  -2: dim_in too large for LDS */
int mid_resample_u8(mid_stream s, const uint8_t *src, const int *boxes, float *out, int n, int dim_in, int dim_out);
/* the same boxes scaled to virt^2 as Pillow's Image.resize(BILINEAR) scales bytes (antialiased; include/resnet_mi.h), of which the window of
 * rows [win_row, + dim_out) x columns [win_col, + dim_out) is written.  -1: sizes, alignment, a window that leaves [0, virt]; -2: LDS */
int mid_resample_aa_u8(mid_stream s, const uint8_t *src, const int *boxes, float *out, int n, int dim_in, int dim_out, int virt, int win_row,
                       int win_col);
/* mixup / CutMix in place on fp32 NCHW images [n][3][dim][dim], row i paired with row n - 1 - i (the middle row of an odd n is not touched).
 * mode 0: nothing is launched.  1: a' = lam a + (1.f - lam) b and b' likewise, every operation rounded on its own.  2: the box rows
 * [y0, y1) x columns [x0, x1) of every plane changes places, clamped into the image on the device; an empty box launches nothing.
 * -1: n outside [1, 65535], image_size != 3 dim^2, NULL or misaligned images, unknown mode, lam outside [0, 1] */
int mid_mix_batch(mid_stream s, float *images, int n, size_t image_size, int dim, int mode, float lam, int y0, int x0, int y1, int x1);
/* labels_b[i] = labels[n - 1 - i] */
int mid_mix_labels(mid_stream s, const int *labels, int *labels_b, int n);
void mid_mix_geometry(size_t out[3]); /* [0] threads, [1] the cap on grid.x, [2] waves of a workgroup (a wave takes one row segment of a CutMix box) */
/* random erasing in place on fp32 NCHW images [n][3][dim][dim]: row i's box boxes_host[4 i ..] = (y0, x0, h, w) (host memory, read before
 * the call returns; clamped into the image) filled with value[c] (mode 0) or value[c] + std[c] z (mode 1; z from noise_seed, first_row + i
 * and the element's position; include/resnet_mi.h).  The boxes travel as kernel arguments, 256 rows a launch; a launch without a box is
 * skipped.  -1: n outside [1, 65535], image_size != 3 dim^2, a NULL pointer, misaligned images, and what mid_erase_fill_ok refuses */
int mid_erase_batch(mid_stream s, float *images, int n, size_t image_size, int dim, const int *boxes_host, int mode, const float *value,
                    const float *std, uint64_t noise_seed, int64_t first_row);
int mid_erase_fill_ok(const char *who, int mode, const float *value, const float *std); /* 0 with the error recorded: unknown mode, a value or std not finite, a negative std */
void mid_erase_geometry(size_t out[4]); /* [0] threads, [1] the cap on grid.x, [2] waves of a workgroup (a wave takes one row segment of a box), [3] rows of a launch */
/* TrivialAugmentWide in place on fp32 NCHW images [n][3][dim][dim] (include/resnet_mi.h, "TrivialAugmentWide"): row i under rows_host[i]
 * (host memory, read before the call returns; mid_ta_row is MiTaRow of resnet_mi.h, the op numbers MI_TA_* there), workspace
 * mid_ta_workspace_bytes(n, dim) bytes of device memory, 16-byte aligned.  The records travel as kernel arguments, 128 rows a launch: a
 * stage and an apply launch per 128 rows (none for 128 identity rows), in front of them one memset of the statistics on the stream when
 * a row needs them.  -1: n outside [1, 65535], dim outside [1, 4096], image_size != 3 dim^2, a NULL pointer, misaligned images or
 * workspace, an op or bin out of range */
typedef struct { int op, bin, neg, arg; double magnitude; float factor; int A[6]; } mid_ta_row;
enum { MID_TA_IDENTITY = 0, MID_TA_SHEAR_X, MID_TA_SHEAR_Y, MID_TA_TRANSLATE_X, MID_TA_TRANSLATE_Y, MID_TA_ROTATE, MID_TA_BRIGHTNESS, MID_TA_COLOR,
       MID_TA_CONTRAST, MID_TA_SHARPNESS, MID_TA_POSTERIZE, MID_TA_SOLARIZE, MID_TA_AUTOCONTRAST, MID_TA_EQUALIZE, MID_TA_OPS = 14, MID_TA_BINS = 31 };
size_t mid_ta_workspace_bytes(int n, int dim);
int mid_trivial_augment(mid_stream s, float *images, int n, size_t image_size, int dim, const mid_ta_row *rows_host, void *workspace);
void mid_ta_geometry(size_t out[4]); /* [0] threads, [1] the cap on grid.x, [2] rows of a launch, [3] pixels a thread takes per turn on the 16-byte path */
/* splitmix64 counter streams on device (synthetic batches): uniform in [lo,hi) / labels mod n_classes */
int mid_fill_uniform(mid_stream s, float *out, size_t n, uint64_t seed, uint64_t offset, float lo, float hi);
/* test aids (kernels_misc.hip; callers serialise): `word` into every LDS word of every CU between two device synchronises, and a read-only
 * pass of the same geometry: out[0] workgroups run, [1] distinct CUs seen, [2] words examined, [3] words != word */
int mid_lds_fill(uint32_t word);
int mid_lds_probe(uint32_t word, size_t out[4]);
int mid_lds_geometry(size_t out[3]); /* [0] LDS bytes per workgroup of the two, [1] CUs of the device, [2] workgroups per launch */
/* the same two under the lock of the fill-after-every-launch mode (runtime.hip), the mode's switch and its counter */
int mid_debug_lds_fill(uint32_t word);
int mid_debug_lds_probe(uint32_t word, size_t out[4]);
int mid_debug_lds_geometry(size_t out[3]);
int mid_debug_lds_fill_mode(int on, uint32_t word);
size_t mid_debug_lds_fills(void);
int mid_fill_labels(mid_stream s, int *out, size_t n, uint64_t seed, uint64_t offset, int n_classes);

/* ---- RCCL (resolved with dlopen at first use) ---- */
int mid_rccl_unique_id_bytes(void);
int mid_rccl_get_unique_id(void *out, int bytes);
void *mid_rccl_comm_init(int rank, int world, const void *unique_id, int bytes);
int mid_rccl_allreduce_sum(void *comm, float *buf, size_t count, mid_stream s);
void mid_rccl_comm_destroy(void *comm);
void mid_rccl_comm_abort(void *comm);

#ifdef __cplusplus
}
#endif
#endif
