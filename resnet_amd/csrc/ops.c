/*
 * ops.c -- operator layer of the C-ABI (the prepareAndDo* wrappers of resnet.cu:1386-1509 as callable
 * entry points): each call runs one kernel family on the library's compute stream with a private
 * workspace and returns after the stream has drained.  Used by the parity tests to drive every HIP
 * kernel on its own.  The convolution operators plan one layer with their routes forced and run it
 * through the runners the trainer runs its table through (layer.c).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "mi_host.h"

/* MI_GUARD bytes of slack on both sides: the bf16 convolution operators read tap-shifted operands with 16-byte loads that may
 * start a few elements before / end a few elements past a tensor (masked lanes); tensors handed to mi_op_*_bf16 must come
 * from here */
void *mi_malloc(size_t bytes) {
    char *p = (char *)mid_malloc(bytes + 2 * MI_GUARD);
    return p ? p + MI_GUARD : NULL;
}
void mi_free(void *p) { if (p) mid_free((char *)p - MI_GUARD); }

static int finish(int rc) {
    mid_stream_sync(mi_global()->compute);
    if (rc) return rc;
    return mid_last_error()[0] ? -1 : 0;
}

/* ---- the convolution operators: plan the layer with the operator's routes, allocate at the planner's sizes, run the module's
 * runners, synchronise, free.  rc: the first failing step's code (later steps are skipped) ---- */
typedef struct { MiLayer L; MiLayerWs w; mid_wt_entry we; mid_stream s; int rc; } OpConv;
/* an operator's routes are forced and its dgrad + BN' fuses wherever the launch can; of the environment only the two switches that choose
 * the kernel inside a route reach it (RESNET_MI_IGEMM, RESNET_MI_BF16_PW_WGRAD) */
static MiOptions op_options(void) {
    MiOptions env, o = {.bnfuse_bwd = 1, .bnfuse_bwd_f32 = 7};
    mi_read_options(&env);
    o.igemm = env.igemm; o.pw_wgrad = env.pw_wgrad;
    return o;
}
/* -2: a route refuses the shape (nothing was allocated).  No weight table here: the NCHW routes re-lay their own weights into the
 * workspace, the channel-last ones get theirs from mi_layer_own_weights (a weight gradient reads none) */
static int op_open(OpConv *o, int dt, const MiOptions *opt, const float *w, int N, int C, int H, int K, int k, int stride, int fwd, int dgrad,
                   int wgrad, int site) {
    const int force[3] = {fwd, dgrad, wgrad};
    MiLayerNeed need = {0, 0, 0, 0};
    memset(o, 0, sizeof *o);
    mi_layer_init(&o->L, w, C, H, K, k, stride);
    if (mi_layer_plan(&o->L, dt, MI_STORE_FAST, opt, N, site, force)) return -2; /* (host only: a refusal touches no device) */
    o->s = mi_global()->compute;
    mi_layer_need(&o->L, &need);
    mi_layer_alloc(NULL, &o->L);
    mi_layer_ws_alloc(NULL, &o->w, &need);
    if (wgrad == MI_NOT_RUN) o->rc = mi_layer_own_weights(&o->L, &o->we, o->s);
    return 0;
}
static int op_close(OpConv *o) {
    const int rc = finish(o->rc);
    mi_layer_free(&o->L);
    mi_layer_ws_free(&o->w);
    return rc;
}
/* one operation of one layer: the weight gradient (out = dw) where a wgrad route is given, else the dgrad (out = dx), else the forward */
static int op_conv(int dt, int fwd, int dgrad, int wgrad, const void *x, const float *w, const void *dy, void *out, const void *addend, int N,
                   int C, int H, int K, int k, int stride) {
    OpConv o;
    const MiOptions opt = op_options();
    if (op_open(&o, dt, &opt, w, N, C, H, K, k, stride, fwd, dgrad, wgrad, 0)) return -2;
    if (wgrad != MI_NOT_RUN) {
        if (o.L.cl) o.rc = mi_layer_x_relayout(&o.L, o.s, x);
        if (!o.rc) o.rc = mi_layer_dy_relayout(&o.L, o.s, dy);
        if (!o.rc) o.rc = mi_layer_wgrad(&o.L, &o.w, o.s, x, dy, (float *)out);
    } else if (dgrad != MI_NOT_RUN) {
        if (!o.rc) o.rc = mi_layer_dy_relayout(&o.L, o.s, dy);
        if (!o.rc) o.rc = mi_layer_dgrad(&o.L, &o.w, o.s, dy, out, addend, NULL, NULL);
    } else if (!o.rc) o.rc = mi_layer_fwd(&o.L, &o.w, o.s, x, out, NULL);
    return op_close(&o);
}
#define OFF MI_NOT_RUN
int mi_op_conv_fwd(const float *x, const float *w, float *y, int N, int C, int H, int K, int k, int stride) {
    return op_conv(MID_F32, MI_FWD_F32, OFF, OFF, x, w, NULL, y, NULL, N, C, H, K, k, stride);
}
int mi_op_conv_dgrad(const float *w, const float *dy, float *dx, int N, int C, int H, int K, int k, int stride, int to_add) {
    return op_conv(MID_F32, OFF, MI_DG_F32, OFF, NULL, w, dy, dx, to_add ? dx : NULL, N, C, H, K, k, stride);
}
int mi_op_conv_wgrad(const float *x, const float *dy, float *dw, int N, int C, int H, int K, int k, int stride) {
    return op_conv(MID_F32, OFF, OFF, MI_WG_F32, x, NULL, dy, dw, NULL, N, C, H, K, k, stride);
}
int mi_op_bn_fwd(const float *x, const float *gamma, const float *beta, float *means, float *vars, float *y, int N, int C,
                 int H, float eps, int relu) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_fwd(mi_global()->compute, ws, x, gamma, beta, NULL, means, vars, y, NULL, NULL, N, C, H * H, eps, relu));
    mid_free(ws);
    return rc;
}
int mi_op_bn_fwd_add_relu(const float *x, const float *gamma, const float *beta, const float *residual, float *means,
                          float *vars, float *y, int N, int C, int H, float eps) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_fwd(mi_global()->compute, ws, x, gamma, beta, residual, means, vars, y, NULL, NULL, N, C, H * H, eps, 0));
    mid_free(ws);
    return rc;
}
int mi_op_bn_bwd(const float *x, const float *gamma, const float *beta, const float *means, const float *vars,
                 const float *dy, const float *mask_src, float *dx, float *dgamma, float *dbeta, int N, int C, int H,
                 float eps, int mask_mode) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_bwd(mi_global()->compute, ws, x, gamma, beta, means, vars, dy, mask_src, dx, dgamma, dbeta, N, C, H * H, eps, mask_mode));
    mid_free(ws);
    return rc;
}
int mi_op_bn_bwd_gate(const float *x, const float *gamma, const float *beta, const float *means, const float *vars,
                      const float *dy, const float *mask_src, float *gated_out, float *dx, float *dgamma, float *dbeta, int N,
                      int C, int H, float eps) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_bwd_gate(mi_global()->compute, ws, x, gamma, beta, means, vars, dy, mask_src, gated_out, dx, dgamma, dbeta, N, C, H * H, eps));
    mid_free(ws);
    return rc;
}
int mi_op_maxpool_fwd(const float *x, float *y, int *max_inds, int N, int C, int H, int k, int stride) {
    return finish(mid_maxpool_fwd(mi_global()->compute, x, y, max_inds, N, C, H, k, stride));
}
int mi_op_maxpool_bwd(const int *max_inds, const float *dy, float *dx, int N, int C, int H, int k, int stride) {
    return finish(mid_maxpool_bwd(mi_global()->compute, max_inds, dy, dx, N, C, H, k, stride));
}
int mi_op_avgpool_fwd(const float *x, float *y, int N, int C, int H) { return finish(mid_avgpool_fwd(mi_global()->compute, x, y, N, C, H * H)); }
int mi_op_avgpool_bwd(const float *dy, float *dx, int N, int C, int H) { return finish(mid_avgpool_bwd(mi_global()->compute, dy, dx, N, C, H * H)); }
int mi_op_relu_deriv(const float *x, const float *up, float *out, size_t n) { return finish(mid_relu_deriv(mi_global()->compute, x, up, out, n)); }
int mi_op_matmul(const float *A, const float *B, float *out, int m, int k, int n) { return finish(mid_gemm_nn(mi_global()->compute, A, B, out, m, k, n)); }
int mi_op_matmul_lt(const float *A_kxm, const float *B, float *out, int m, int k, int n) { return finish(mid_gemm_tn(mi_global()->compute, A_kxm, B, out, m, k, n)); }
int mi_op_matmul_rt(const float *A, const float *B_nxk, float *out, int m, int k, int n) { return finish(mid_gemm_nt(mi_global()->compute, A, B_nxk, out, m, k, n)); }
int mi_op_softmax(const float *x, float *out, int N, int L) { return finish(mid_softmax(mi_global()->compute, x, out, N, L)); }
int mi_op_ce_deriv(const float *pred, const int *labels, float *d, int N, int L) { return finish(mid_ce_deriv(mi_global()->compute, pred, labels, d, N, L)); }
_Static_assert(sizeof(MiLossMetrics) == sizeof(mid_loss_metrics), "one record, declared on both sides of mi_device.h");
/* the argument rules mi_op_loss_head and mi_trainer_set_loss share; 0, or -1 with mi_last_error set */
int mi_loss_args_ok(const char *who, float smoothing, int topk, int L) {
    if (!(smoothing >= 0.f && smoothing < 1.f)) { mi_record_host_error(who, "smoothing lies in [0, 1)"); return -1; }
    if (topk < 1 || topk > L) { mi_record_host_error(who, "topk lies in [1, number of classes]"); return -1; }
    return 0;
}
int mi_op_loss_head(const float *logits, const int *labels, float *pred, float *dlogits, float *row_loss, int *row_rank, int N, int L,
                    float smoothing, int topk, MiLossMetrics *last_dev, MiLossMetrics *total_dev) {
    if (N < 1 || L < 1) { mi_record_host_error("mi_op_loss_head", "N and L are at least 1"); return -1; }
    if (mi_loss_args_ok("mi_op_loss_head", smoothing, topk, L)) return -1;
    /* the totals are reduced from the row values: rows the caller does not want live in scratch */
    const int totals = last_dev || total_dev;
    float *rl = totals && !row_loss ? (float *)mid_malloc((size_t)N * sizeof(float)) : NULL;
    int *rr = totals && !row_rank ? (int *)mid_malloc((size_t)N * sizeof(int)) : NULL;
    const int rc = finish(mid_loss_head(mi_global()->compute, logits, labels, pred, dlogits, row_loss ? row_loss : rl, row_rank ? row_rank : rr, N, L,
                                        smoothing, topk, (mid_loss_metrics *)last_dev, (mid_loss_metrics *)total_dev));
    mid_free(rl); mid_free(rr);
    return rc;
}
int mi_op_loss_head_mix(const float *logits, const int *labels_a, const int *labels_b, float lam, float *pred, float *dlogits, float *row_loss,
                        int *row_rank, int N, int L, float smoothing, int topk, MiLossMetrics *last_dev, MiLossMetrics *total_dev) {
    const char *who = "mi_op_loss_head_mix";
    if (N < 1 || L < 1) { mi_record_host_error(who, "N and L are at least 1"); return -1; }
    if (mi_loss_args_ok(who, smoothing, topk, L)) return -1;
    if (!(lam >= 0.f && lam <= 1.f)) { mi_record_host_error(who, "lam lies in [0, 1]"); return -1; }
    if (!labels_b) { mi_record_host_error(who, "labels_b is NULL"); return -1; }
    const int totals = last_dev || total_dev;
    float *rl = totals && !row_loss ? (float *)mid_malloc((size_t)N * sizeof(float)) : NULL;
    int *rr = totals && !row_rank ? (int *)mid_malloc((size_t)N * sizeof(int)) : NULL;
    const int rc = finish(mid_loss_head_mix(mi_global()->compute, logits, labels_a, labels_b, lam, pred, dlogits, row_loss ? row_loss : rl,
                                            row_rank ? row_rank : rr, N, L, smoothing, topk, (mid_loss_metrics *)last_dev, (mid_loss_metrics *)total_dev));
    mid_free(rl); mid_free(rr);
    return rc;
}
/* n / (n - 1) of a batch-norm layer whose statistics are taken over n samples per channel, in double, stored as float; 1 where n <= 1 */
float mi_bn_unbias(int64_t n) { return n > 1 ? (float)((double)n / (double)(n - 1)) : 1.f; }
/* bn_running_update_kernel on its own: the table built and checked here (layer i at the sum of the channel counts before it) */
int mi_op_bn_running_update(const float *const *means_dev, const float *const *vars_dev, const int *channels, const int64_t *counts, int n_layers,
                            float *running_dev, int running_channels, float momentum) {
    const char *who = "mi_op_bn_running_update";
    if (!(momentum > 0.f && momentum <= 1.f)) { mi_record_host_error(who, "momentum lies in (0, 1]"); return -1; }
    if (n_layers < 1 || !means_dev || !vars_dev || !channels || !counts || !running_dev) { mi_record_host_error(who, "at least one layer, no NULL array"); return -1; }
    int64_t sum = 0;
    for (int i = 0; i < n_layers; i++) {
        if (channels[i] < 1 || !means_dev[i] || !vars_dev[i]) { mi_record_host_error(who, "every layer has at least one channel and both statistics"); return -1; }
        if (counts[i] < 1) { mi_record_host_error(who, "every count is at least 1"); return -1; }
        sum += channels[i];
    }
    if (sum > (int64_t)running_channels) { mi_record_host_error(who, "the layers' channels exceed running_channels"); return -1; }
    mid_bn_run_entry *tab = (mid_bn_run_entry *)malloc(sizeof(mid_bn_run_entry) * (size_t)n_layers);
    int first = 0;
    for (int i = 0; i < n_layers; i++) {
        tab[i].means = means_dev[i]; tab[i].vars = vars_dev[i]; tab[i].first = tab[i].off = first; tab[i].C = channels[i];
        tab[i].unbias = mi_bn_unbias(counts[i]);
        first += channels[i];
    }
    mid_stream s = mi_global()->compute;
    mid_bn_run_entry *tab_dev = (mid_bn_run_entry *)mid_malloc(sizeof(mid_bn_run_entry) * (size_t)n_layers);
    if (!tab_dev) { free(tab); return -3; }
    mid_memcpy_h2d(tab_dev, tab, sizeof(mid_bn_run_entry) * (size_t)n_layers, s);
    const int rc = finish(mid_bn_running_update(s, tab_dev, n_layers, (int)sum, running_dev, (size_t)running_channels, momentum));
    mid_free(tab_dev);
    free(tab);
    return rc;
}
int mi_op_adam(float *p, const float *g, float *m, float *v, size_t n, float lr, float wd, float b1, float b2, float cur_b1,
               float cur_b2, float eps, int *nan_flag_dev) {
    return finish(mid_adam(mi_global()->compute, p, (float *)g, m, v, n, lr, wd, b1, b2, cur_b1, cur_b2, eps, nan_flag_dev, 0, NULL, 0, 0));
}
int mi_op_momentum_update2(int kind, float *p, float *g, float *b, size_t n, const size_t *offsets_host, int n_tensors,
                           const int *tensor_is_weight_host, float lr, float wd, float wd_norm, float momentum, float trust_coef, int *nan_flag_dev,
                           double *sq_norms_out_host) {
    if (kind != MI_OPT_SGD && kind != MI_OPT_LARS) { mi_record_host_error("mi_op_momentum_update", "kind is MI_OPT_SGD or MI_OPT_LARS"); return -1; }
    if (!(wd_norm >= 0.f) || isinf(wd_norm)) { mi_record_host_error("mi_op_momentum_update", "wd_norm is finite and >= 0"); return -1; }
    if (n_tensors < 1 || offsets_host[n_tensors] > n) { mi_record_host_error("mi_op_momentum_update", "tensors beyond the n floats"); return -1; }
    int *sizes = (int *)malloc(sizeof(int) * (size_t)n_tensors);
    for (int i = 0; i < n_tensors; i++) {
        const size_t len = offsets_host[i + 1] >= offsets_host[i] ? offsets_host[i + 1] - offsets_host[i] : 0;
        sizes[i] = len > (size_t)INT32_MAX ? -1 : (int)len; /* descending or oversized: refused by mi_optim_init */
    }
    MiOptim o;
    int rc = mi_optim_init(&o, kind, momentum, trust_coef, offsets_host, sizes, tensor_is_weight_host, n_tensors);
    free(sizes);
    if (rc) return -1;
    mid_stream s = mi_global()->compute;
    rc = finish(mi_optim_step(&o, s, p, g, b, 0, offsets_host[n_tensors], lr, wd, wd_norm, nan_flag_dev, sq_norms_out_host != NULL));
    if (!rc && sq_norms_out_host) {
        mid_memcpy_d2h(sq_norms_out_host, o.sq_dev, 2 * sizeof(double) * (size_t)n_tensors, s);
        rc = finish(0);
    }
    mi_optim_free(&o);
    return rc;
}
int mi_op_momentum_update(int kind, float *p, float *g, float *b, size_t n, const size_t *offsets_host, int n_tensors,
                          const int *tensor_is_weight_host, float lr, float wd, float momentum, float trust_coef, int *nan_flag_dev,
                          double *sq_norms_out_host) {
    return mi_op_momentum_update2(kind, p, g, b, n, offsets_host, n_tensors, tensor_is_weight_host, lr, wd, wd, momentum, trust_coef, nan_flag_dev,
                                  sq_norms_out_host);
}
_Static_assert(sizeof(MiClipRecord) == sizeof(mid_clip_record), "one record, declared on both sides of mi_device.h");
/* gradient clipping (resnet_mi.h): the three kernels on their own.  Every refusal comes before any device work */
int mi_op_clip_grad_norm(float *g, size_t n, const size_t *offsets_host, int n_tensors, float max_norm, MiClipRecord *out) {
    const char *who = "mi_op_clip_grad_norm";
    if (!g || ((uintptr_t)g & 15) != 0) { mi_record_host_error(who, "g is a 16-byte aligned device pointer"); return -1; }
    if (n == 0) { mi_record_host_error(who, "n is at least 1"); return -1; }
    if (!(max_norm > 0.f) || isinf(max_norm)) { mi_record_host_error(who, "max_norm is finite and > 0"); return -1; }
    if (!offsets_host || n_tensors < 1 || offsets_host[n_tensors] > n) { mi_record_host_error(who, "tensors beyond the n floats"); return -1; }
    int *sizes = (int *)malloc(sizeof(int) * (size_t)n_tensors);
    for (int i = 0; i < n_tensors; i++) {
        const size_t len = offsets_host[i + 1] >= offsets_host[i] ? offsets_host[i + 1] - offsets_host[i] : 0;
        sizes[i] = len > (size_t)INT32_MAX || offsets_host[i + 1] < offsets_host[i] ? -1 : (int)len; /* descending or oversized: refused by the chunk cutting */
    }
    MiClip k;
    int rc = mi_clip_init(&k, who, offsets_host, sizes, n_tensors);
    free(sizes);
    if (rc) return -1;
    mid_stream s = mi_global()->compute;
    rc = finish(mi_clip_run(&k, s, g, max_norm));
    if (!rc && out) {
        mid_memcpy_d2h(out, k.rec_dev, sizeof *out, s);
        rc = finish(0);
    }
    mi_clip_free(&k);
    return rc;
}
/* tools/bench_clip.py: the mean time in ms of one launch of the norm (pass 0), coefficient (1) or scale (2) kernel over `reps` launches
 * behind 3 unmeasured ones, each between HIP events on the compute stream (mi_prof_*, which it switches off again); the record the scale
 * kernel reads comes from one norm + coefficient pass in front.  Arguments as mi_op_clip_grad_norm; < 0: refused or failed */
double mi_debug_clip_pass_ms(int pass, float *g, size_t n, const size_t *offsets_host, int n_tensors, float max_norm, int reps) {
    const char *who = "mi_debug_clip_pass_ms";
    if (pass < 0 || pass > 2 || reps < 1) { mi_record_host_error(who, "pass is 0, 1 or 2 and reps >= 1"); return -1.0; }
    if (!g || ((uintptr_t)g & 15) != 0 || n == 0 || !offsets_host || n_tensors < 1 || offsets_host[n_tensors] > n || !(max_norm > 0.f) || isinf(max_norm)) {
        mi_record_host_error(who, "arguments as mi_op_clip_grad_norm");
        return -1.0;
    }
    int *sizes = (int *)malloc(sizeof(int) * (size_t)n_tensors);
    for (int i = 0; i < n_tensors; i++) {
        const size_t len = offsets_host[i + 1] >= offsets_host[i] ? offsets_host[i + 1] - offsets_host[i] : 0;
        sizes[i] = len > (size_t)INT32_MAX || offsets_host[i + 1] < offsets_host[i] ? -1 : (int)len;
    }
    MiClip k;
    int rc = mi_clip_init(&k, who, offsets_host, sizes, n_tensors);
    free(sizes);
    if (rc) return -1.0;
    mid_stream s = mi_global()->compute;
    rc = mid_clip_norm(s, g, k.chunks_dev, k.n_chunks, k.part_dev) || mid_clip_coef(s, k.part_dev, k.n_chunks, max_norm, k.rec_dev);
    double ms = 0.0;
    for (int i = -3; i < reps && !rc; i++) {
        if (i == 0) { mid_stream_sync(s); mid_prof_enable(1 << 4); mid_prof_reset(); } /* family 4: other */
        rc = pass == 0 ? mid_clip_norm(s, g, k.chunks_dev, k.n_chunks, k.part_dev)
           : pass == 1 ? mid_clip_coef(s, k.part_dev, k.n_chunks, max_norm, k.rec_dev) : mid_clip_scale(s, g, k.chunks_dev, k.n_chunks, k.rec_dev);
    }
    rc = finish(rc);
    mid_prof_get(4, NULL, &ms, NULL, NULL);
    mid_prof_enable(0);
    mi_clip_free(&k);
    return rc ? -1.0 : ms / reps;
}
/* weight averaging (resnet_mi.h): the weight of update k, host only; the two kernels on their own (the launchers refuse what the header lists) */
float mi_ema_weight(double decay, int warmup, int64_t k) {
    double d = decay;
    if (warmup) {
        const double ramp = (1.0 + (double)k) / (10.0 + (double)k);
        if (ramp < d) d = ramp;
    }
    return (float)(1.0 - d);
}
int mi_op_ema_update(float *ema, const float *p, size_t n, float w) { return finish(mid_ema_update(mi_global()->compute, ema, p, n, w)); }
int mi_op_exchange(float *a, float *b, size_t n) { return finish(mid_exchange(mi_global()->compute, a, b, n)); }
void mi_debug_ema_geometry(size_t out[4]) { mid_ema_geometry(out); }
/* gradient accumulation (resnet_mi.h): the kernel on its own; it runs in the geometry of the two above */
int mi_op_grad_accumulate(float *acc, float *g, size_t n, int mode, float scale) { return finish(mid_grad_accumulate(mi_global()->compute, acc, g, n, mode, scale)); }
void mi_debug_accum_geometry(size_t out[4]) { mid_ema_geometry(out); }
int mi_op_nhwc_to_nchw(const float *in,float *out, int N, int H, int W, int C) { return finish(mid_nhwc_to_nchw(mi_global()->compute, in, out, N, H, W, C)); }
int mi_op_decode_u8(const uint8_t *src_dev, const int *plan_dev, float *out_nchw, int n, int dim_in, int dim_out) {
    return finish(mid_decode_u8(mi_global()->compute, src_dev, plan_dev, out_nchw, n, dim_in, dim_out));
}
int mi_op_resample_u8(const uint8_t *src_dev, const int *boxes_dev, float *out_nchw, int n, int dim_in, int dim_out) {
    return finish(mid_resample_u8(mi_global()->compute, src_dev, boxes_dev, out_nchw, n, dim_in, dim_out));
}
int mi_op_resample_aa_u8(const uint8_t *src_dev, const int *boxes_dev, float *out_nchw, int n, int dim_in, int dim_out, int virt, int win_row,
                         int win_col) {
    return finish(mid_resample_aa_u8(mi_global()->compute, src_dev, boxes_dev, out_nchw, n, dim_in, dim_out, virt, win_row, win_col));
}
int mi_op_mix_batch(float *images_nchw, int n, int image_size, int dim, const MiMixPlan *plan_host) {
    if (!plan_host) { mi_record_host_error("mi_op_mix_batch", "plan_host is NULL"); return -1; }
    if (image_size < 1) { mi_record_host_error("mi_op_mix_batch", "image_size = 3 dim^2"); return -1; }
    return finish(mid_mix_batch(mi_global()->compute, images_nchw, n, (size_t)image_size, dim, plan_host->mode, plan_host->lam, plan_host->y0,
                                plan_host->x0, plan_host->y1, plan_host->x1));
}
void mi_debug_mix_geometry(size_t out[3]) { mid_mix_geometry(out); }
int mi_op_erase_batch(float *images_nchw, int n, int image_size, int dim, const int *boxes_host, const MiEraseFill *fill_host, int64_t first_row) {
    if (!boxes_host || !fill_host) { mi_record_host_error("mi_op_erase_batch", "boxes_host / fill_host is NULL"); return -1; }
    if (image_size < 1) { mi_record_host_error("mi_op_erase_batch", "image_size = 3 dim^2"); return -1; }
    return finish(mid_erase_batch(mi_global()->compute, images_nchw, n, (size_t)image_size, dim, boxes_host, fill_host->mode, fill_host->value,
                                  fill_host->std, fill_host->noise_seed, first_row));
}
void mi_debug_erase_geometry(size_t out[4]) { mid_erase_geometry(out); }
_Static_assert(sizeof(MiTaRow) == sizeof(mid_ta_row), "MiTaRow and mid_ta_row are one layout");
size_t mi_ta_workspace_bytes(int n, int dim) { return mid_ta_workspace_bytes(n, dim); }
int mi_op_trivial_augment(float *images_nchw, int n, int image_size, int dim, const MiTaRow *rows_host, void *workspace_dev) {
    if (!rows_host || !workspace_dev) { mi_record_host_error("mi_op_trivial_augment", "rows_host / workspace_dev is NULL"); return -1; }
    if (image_size < 1) { mi_record_host_error("mi_op_trivial_augment", "image_size = 3 dim^2"); return -1; }
    return finish(mid_trivial_augment(mi_global()->compute, images_nchw, n, (size_t)image_size, dim, (const mid_ta_row *)rows_host, workspace_dev));
}
void mi_debug_ta_geometry(size_t out[4]) { mid_ta_geometry(out); }
int mi_op_fill_uniform(float *out, size_t n, uint64_t seed, float lo, float hi) { return finish(mid_fill_uniform(mi_global()->compute, out, n, seed, 0, lo, hi)); }
int mi_debug_lds_fill(uint32_t word) { return finish(mid_debug_lds_fill(word)); }
int mi_debug_poison_lds(void) { return mi_debug_lds_fill(0xFFFFFFFFu); }
int mi_debug_lds_probe(uint32_t word, size_t out[4]) { return finish(mid_debug_lds_probe(word, out)); }
int mi_debug_lds_geometry(size_t out[3]) { return finish(mid_debug_lds_geometry(out)); }
int mi_debug_lds_fill_mode(int on, uint32_t word) { return finish(mid_debug_lds_fill_mode(on, word)); }
size_t mi_debug_lds_fills(void) { return mid_debug_lds_fills(); }
int mi_debug_redzone(size_t zone_bytes, int fill_byte) { return mid_redzone(zone_bytes, fill_byte); }
int mi_debug_redzone_check(void) { return mid_redzone_check(); }
void mi_debug_redzone_stats(size_t *allocs_checked, size_t *zone_bytes_checked, size_t *live) { mid_redzone_stats(allocs_checked, zone_bytes_checked, live); }
int mi_debug_trace_names(char *buf, size_t cap) { return mid_trace_names(buf, cap); }
void mi_debug_trace_clear(void) { mid_trace_clear(); }
/* 1: the fp32 operator of this shape runs operation op on the implicit GEMM (the planner's answer under the process's switches) */
static int on_igemm(int op, int N, int C, int H, int K, int k, int stride) {
    const MiOptions opt = op_options();
    return op >= 0 && op <= 2 && mi_layer_f32_kernel(&opt, op, N, C, H, K, k, stride) == MI_K_IGEMM;
}
int mi_debug_conv_plan(int op, int N, int C, int H, int K, int k, int stride, int out[9]) {
    if (on_igemm(op, N, C, H, K, k, stride)) return mid_igemm_plan(op, N, C, H, K, k, stride, out);
    for (int i = 0; i < 9; i++) out[i] = 0;
    return 0;
}
int mi_conv_plan(int dtype, int route, int op, int N, int C, int H, int K, int k, int stride, int out[7]) {
    for (int i = 0; i < 7; i++) out[i] = 0;
    int ok = 0;
    if (op < 0 || op > 2) ok = 0;
    else if (dtype == MI_DTYPE_F32 && route == MI_ROUTE_DEFAULT) ok = on_igemm(op, N, C, H, K, k, stride) && mid_igemm_conv_plan(op, N, C, H, K, k, stride, out);
    else if (dtype == MI_DTYPE_BF16 && route == MI_ROUTE_DEFAULT) ok = mid_bf16_conv_plan(op, N, C, H, K, k, stride, out);
    else if (dtype == MI_DTYPE_BF16 && route >= MI_ROUTE_CL && route <= MI_ROUTE_PW) ok = mid_cl_conv_plan(route, op, N, C, H, K, k, stride, out);
    if (!ok) { for (int i = 0; i < 7; i++) out[i] = 0; return -2; }
    return 0;
}

/* ---- typed operators: activation tensors as bf16 (MI_DTYPE_BF16), arithmetic in fp32 ---- */
int mi_op_convert(const void *in, int in_dt, void *out, int out_dt, size_t n) {
    if (in_dt == MID_F32 && out_dt == MID_BF16) return finish(mid_f32_to_bf16(mi_global()->compute, (const float *)in, out, n));
    if (in_dt == MID_BF16 && out_dt == MID_F32) return finish(mid_bf16_to_f32(mi_global()->compute, in, (float *)out, n));
    return -2;
}
int mi_op_conv_fwd_bf16(const void *x, const float *w, void *y, int N, int C, int H, int K, int k, int stride) {
    return op_conv(MID_BF16, MI_FWD_BF16, OFF, OFF, x, w, NULL, y, NULL, N, C, H, K, k, stride);
}
int mi_op_conv_dgrad_bf16(const float *w, const void *dy, void *dx, int N, int C, int H, int K, int k, int stride, int to_add) {
    return op_conv(MID_BF16, OFF, MI_DG_BF16, OFF, NULL, w, dy, dx, to_add ? dx : NULL, N, C, H, K, k, stride);
}
int mi_op_conv_wgrad_bf16(const void *x, const void *dy, float *dw, int N, int C, int H, int K, int k, int stride) {
    return op_conv(MID_BF16, OFF, OFF, MI_WG_BF16, x, NULL, dy, dw, NULL, N, C, H, K, k, stride);
}
/* dgrad of one convolution followed by the backward of the batch norm (+ReLU) in front of it, the way backwards_pass chains them
 * (prepreAndDoConvolutionDeriv + activationAndBatchNormDeriv, resnet.cu:1399-1429, 1455-1480): where the launch allows, the dgrad gates its
 * output by mask > 0 and does the BN' reduction pass in its epilogue (bf16 storage: the NCHW kernel; fp32: the stride-1 layers on the
 * implicit-GEMM route).  All image tensors of storage type dt.
 * Returns < 0 on error, else the number of partial rows the dgrad left (0 = the separate reduction pass ran). */
static int op_dgrad_bn_bwd(int dt, const float *w, const void *dy, const void *addend, void *gated, int N, int C, int H, int K, int k, int stride,
                           const void *bn_x, const void *mask, const float *gamma, const float *beta, const float *means, const float *vars,
                           float eps, void *bn_dx, float *dgamma, float *dbeta) {
    OpConv o;
    const size_t bytes = (size_t)N * C * H * H * (dt == MID_BF16 ? 2 : 4);
    mid_bn_bwd_parts fz = {NULL}, req;
    void *tmp = NULL;
    const MiOptions opt = op_options();
    if (op_open(&o, dt, &opt, w, N, C, H, K, k, stride, OFF, dt == MID_BF16 ? MI_DG_BF16 : MI_DG_F32, OFF, 1)) return -2;
    if (addend) mid_memcpy_d2d(gated, addend, bytes, o.s);
    if (!o.rc) o.rc = mi_layer_dgrad(&o.L, &o.w, o.s, dy, gated, addend ? gated : NULL, mi_layer_fz_request(&o.L, &o.w, &req, bn_x, mask, means), &fz);
    const int nparts = fz.nparts;
    /* the unfused chain: BN' gates by the mask itself (mode 3 writes the gated gradient where the fused form leaves it) */
    if (!o.rc && !nparts && !(tmp = mi_malloc(bytes))) o.rc = -3;
    if (!o.rc) o.rc = mi_bn_bwd_unit(&o.w, o.s, &fz, bn_x, dt, gamma, beta, means, vars, gated, mask, 3, tmp, dt, bn_dx, dgamma, dbeta, N, C, H * H, eps);
    if (!o.rc && tmp) mid_memcpy_d2d(gated, tmp, bytes, o.s);
    const int rc = op_close(&o);
    mi_free(tmp);
    return rc < 0 ? rc : nparts;
}
int mi_op_conv_dgrad_bn_bwd_bf16(const float *w, const void *dy, const void *addend, void *gated, int N, int C, int H, int K, int k, int stride,
                                 const void *bn_x, const void *mask, const float *gamma, const float *beta, const float *means,
                                 const float *vars, float eps, void *bn_dx, float *dgamma, float *dbeta) {
    return op_dgrad_bn_bwd(MID_BF16, w, dy, addend, gated, N, C, H, K, k, stride, bn_x, mask, gamma, beta, means, vars, eps, bn_dx, dgamma, dbeta);
}
int mi_op_conv_dgrad_bn_bwd_f32(const float *w, const float *dy, const float *addend, float *gated, int N, int C, int H, int K, int k, int stride,
                                const float *bn_x, const float *mask, const float *gamma, const float *beta, const float *means,
                                const float *vars, float eps, float *bn_dx, float *dgamma, float *dbeta) {
    return op_dgrad_bn_bwd(MID_F32, w, dy, addend, gated, N, C, H, K, k, stride, bn_x, mask, gamma, beta, means, vars, eps, bn_dx, dgamma, dbeta);
}
/* the stem (7x7 stride 2, 3 -> 64) on the matrix cores: exact = 1 in exact fp32 (MI_FWD_STEM_F32, the stem of the fp32 storage mode where
 * RESNET_MI_IGEMM allows the matrix cores), exact = 0 image and weights rounded to bf16 inside (MI_FWD_STEM_BF16).  x fp32; conv_dt =
 * storage type of the stem's own output and of its gradient, a_dt = of the activations behind its BN */
static int stem_open(OpConv *o, const float *w, int N, int H, int exact, int conv_dt, int a_dt, int wgrad) {
    MiOptions opt = op_options();
    opt.stem_tensors_f32 = conv_dt == MID_F32;
    if ((exact || a_dt != MID_BF16) && conv_dt != MID_F32) return -2;
    return op_open(o, a_dt, &opt, w, N, 3, H, 64, 7, 2, exact ? MI_FWD_STEM_F32 : MI_FWD_STEM_BF16, OFF,
                   !wgrad ? OFF : exact ? MI_WG_STEM_F32 : MI_WG_STEM_BF16, 0);
}
static int op_stem_fwd(const float *x, const float *w, float *y, int N, int H, int exact) {
    OpConv o;
    if (stem_open(&o, w, N, H, exact, MID_F32, MID_F32, 0)) return -2;
    if (!o.rc) o.rc = mi_layer_fwd(&o.L, &o.w, o.s, x, y, NULL);
    return op_close(&o);
}
static int op_stem_wgrad(const float *x, const float *w, const void *dy, int dy_dt, float *dw, int N, int H, int exact) {
    OpConv o;
    if (stem_open(&o, w, N, H, exact, dy_dt, dy_dt, 1)) return -2;
    void *y = mi_malloc((size_t)N * 64 * (H / 2) * (H / 2) * (dy_dt == MID_BF16 ? 2 : 4));
    if (!y) o.rc = -3;
    if (!o.rc) o.rc = mi_layer_fwd(&o.L, &o.w, o.s, x, y, NULL); /* leaves the padded planes in xp */
    if (!o.rc) o.rc = mi_layer_wgrad(&o.L, &o.w, o.s, x, dy, dw);
    const int rc = op_close(&o);
    mi_free(y);
    return rc;
}
int mi_op_stem_fwd_bf16(const float *x, const float *w, float *y, int N, int H) { return op_stem_fwd(x, w, y, N, H, 0); }
int mi_op_stem_fwd_f32(const float *x, const float *w, float *y, int N, int H) { return op_stem_fwd(x, w, y, N, H, 1); }
int mi_op_stem_wgrad_bf16(const float *x, const float *w, const float *dy, float *dw, int N, int H) { return op_stem_wgrad(x, w, dy, MID_F32, dw, N, H, 0); }
int mi_op_stem_wgrad_f32(const float *x, const float *w, const float *dy, float *dw, int N, int H) { return op_stem_wgrad(x, w, dy, MID_F32, dw, N, H, 1); }
/* the bf16 stem's weight gradient from dy stored as dy_dt (bf16: the stem tensors of the bf16 trainer, mi_trainer_stem_dtype) */
int mi_op_stem_wgrad_bf16_t(const float *x, const float *w, const void *dy, int dy_dt, float *dw, int N, int H) {
    return op_stem_wgrad(x, w, dy, dy_dt, dw, N, H, 0);
}
/* A convolution and the batch norm behind it the way forward_pass runs the pair (resnet.cu:1386-1396 + 1431-1453; unit_fwd's two calls):
 * the statistics come out of the convolution's own epilogue (fp32 accumulators) where its kernel leaves partials, and from a pass over
 * conv_out where it does not.  Returns < 0 on error, > 0: the statistics were fused (number of partial rows), 0: separate pass */
static int op_conv_bn_fwd(OpConv *o, const void *x, void *conv_out, const float *gamma, const float *beta, float *means, float *vars, void *y,
                          float eps, int relu) {
    mid_bn_parts *parts = &o->w.bn_parts;
    if (!o->rc) o->rc = mi_layer_fwd(&o->L, &o->w, o->s, x, conv_out, parts);
    if (!o->rc) o->rc = mi_layer_bn_fwd(&o->L, &o->w, o->s, parts, conv_out, gamma, beta, NULL, means, vars, y, NULL, NULL, eps, relu, NULL);
    const int nparts = parts->nparts, rc = op_close(o);
    return rc < 0 ? rc : nparts;
}
/* dt = storage type of x, conv_out and y; the layer on the fp32 route of its shape, or the bf16 NCHW kernels */
int mi_op_conv_bn_fwd_t(const void *x, const float *w, void *conv_out, int dt, const float *gamma, const float *beta, float *means,
                        float *vars, void *y, int N, int C, int H, int K, int k, int stride, float eps, int relu) {
    OpConv o;
    const MiOptions opt = op_options();
    if (op_open(&o, dt, &opt, w, N, C, H, K, k, stride, dt == MID_BF16 ? MI_FWD_BF16 : MI_FWD_F32, OFF, OFF, 0)) return -2;
    return op_conv_bn_fwd(&o, x, conv_out, gamma, beta, means, vars, y, eps, relu);
}
/* the same pair on a bf16 3x3 layer whose forward takes the channel-last kernel (MI_FWD_CL): weights re-laid, input re-laid into a zeroed
 * operand, the channel-last forward leaving the statistics partials, the BN behind it.  All image tensors bf16. */
int mi_op_conv_bn_fwd_bf16_cl(const void *x, const float *w, void *conv_out, const float *gamma, const float *beta, float *means,
                              float *vars, void *y, int N, int C, int H, int K, int stride, float eps, int relu) {
    OpConv o;
    const MiOptions opt = op_options();
    if (op_open(&o, MID_BF16, &opt, w, N, C, H, K, 3, stride, MI_FWD_CL, OFF, OFF, 0)) return -2;
    return op_conv_bn_fwd(&o, x, conv_out, gamma, beta, means, vars, y, eps, relu);
}
/* the stem and its BN + ReLU as forward_pass runs them on the matrix cores: exact = 1 MI_FWD_STEM_F32 (conv_out fp32), exact = 0
 * MI_FWD_STEM_BF16 with conv_out fp32 or bf16 (mi_trainer_stem_dtype); a_dt = storage type of y.  The statistics come from the stem
 * kernel's partials.  Returns < 0 on error, else the number of partial rows (0 = separate statistics pass). */
int mi_op_stem_bn_fwd_t(const float *x, const float *w, void *conv_out, int conv_dt, const float *gamma, const float *beta, float *means,
                        float *vars, void *y, int a_dt, int N, int H, float eps, int exact) {
    OpConv o;
    if (stem_open(&o, w, N, H, exact, conv_dt, a_dt, 0)) return -2;
    return op_conv_bn_fwd(&o, x, conv_out, gamma, beta, means, vars, y, eps, 1);
}
int mi_op_bn_fwd_t(const void *x, int x_dt, const float *gamma, const float *beta, const void *residual, float *means, float *vars,
                   void *y, int a_dt, int N, int C, int H, float eps, int relu) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_fwd_t(mi_global()->compute, ws, NULL, x, x_dt, gamma, beta, residual, means, vars, y, a_dt, NULL, NULL, N, C, H * H, eps, relu, NULL, 0));
    mid_free(ws);
    return rc;
}
/* BN (+ residual) + ReLU of a bf16 tensor with the output written twice, as forward_pass does in front of a 3x3: y (bf16 NCHW) and ycl =
 * the same values channel-last -- par = 0: one zero-padded plane [N][H+2][H+2][C] (stride-1 3x3); par = 1: the four parity planes
 * [N][2x2][H/2+1][H/2+1][C] of a stride-2 3x3 (the caller zeroes ycl once: only the interior is written) */
int mi_op_bn_fwd_cl_bf16(const void *x, const float *gamma, const float *beta, const void *residual, float *means, float *vars, void *y, void *ycl,
                         int N, int C, int H, float eps, int par) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_fwd_t(mi_global()->compute, ws, NULL, x, MID_BF16, gamma, beta, residual, means, vars, y, MID_BF16, NULL, NULL, N, C, H * H, eps,
                                 residual ? 0 : 1, ycl, par ? -H : H));
    mid_free(ws);
    return rc;
}
int mi_op_bn_bwd_t(const void *x, int x_dt, const float *gamma, const float *beta, const float *means, const float *vars,
                   const void *dy, const void *mask_src, void *gated_out, int a_dt, void *dx, float *dgamma, float *dbeta, int N, int C,
                   int H, float eps, int mask_mode) {
    float *ws = (float *)mid_malloc(mid_bn_ws_floats(C) * sizeof(float));
    int rc = finish(mid_bn_bwd_t(mi_global()->compute, ws, x, x_dt, gamma, beta, means, vars, dy, mask_src, gated_out, a_dt, dx, dgamma, dbeta, N, C, H * H, eps, mask_mode));
    mid_free(ws);
    return rc;
}
int mi_op_bn_apply_t(const void *x, int x_dt, const float *gamma, const float *beta, const void *residual, const float *means,
                     const float *vars, void *y, int a_dt, int N, int C, int H, float eps, int relu) {
    return finish(mid_bn_apply_t(mi_global()->compute, x, x_dt, gamma, beta, residual, means, vars, y, a_dt, N, C, H * H, eps, relu, NULL, 0));
}
int mi_op_maxpool_fwd_t(const void *x, void *y, int dt, int *max_inds, int N, int C, int H, int k, int stride) {
    return finish(mid_maxpool_fwd_t(mi_global()->compute, x, y, dt, max_inds, N, C, H, k, stride));
}
int mi_op_maxpool_bwd_t(const int *max_inds, const void *dy, void *dx, int dt, int N, int C, int H, int k, int stride) {
    return finish(mid_maxpool_bwd_t(mi_global()->compute, max_inds, dy, dx, dt, N, C, H, k, stride));
}
int mi_op_avgpool_fwd_t(const void *x, int dt, float *y, int N, int C, int H) { return finish(mid_avgpool_fwd_t(mi_global()->compute, x, dt, y, N, C, H * H)); }
int mi_op_avgpool_bwd_t(const float *dy, void *dx, int dt, int N, int C, int H) { return finish(mid_avgpool_bwd_t(mi_global()->compute, dy, dx, dt, N, C, H * H)); }
int mi_bf16_conv_supported(int op, int N, int C, int H, int K, int k, int stride) { return mid_bf16_supported(op, N, C, H, K, k, stride); }
/* 1: the 1x1 weight gradient of this shape runs on the LDS-DMA kernel (pw_wgrad_kernel) inside mi_op_conv_wgrad_bf16 / the bf16 trainer */
int mi_bf16_pw_wgrad_supported(int N, int C, int H, int K) { return mid_pw_wgrad_supported(N, C, H, K); }
void mi_clear_error(void) { mid_clear_error(); }

/* the device-side merge of cross-replica batch norm on R replicas held by one process (see mid_bn_debug_merge): lets a one-GPU
 * box check the merge against whole-batch statistics with two DIFFERENT replicas.  All pointers device, [R][C]; sums_out [R][2C]
 * or NULL; (means, vars) or (dgamma, dbeta) may be NULL to run one half only. */
int mi_debug_bn_merge(int R, int C, float *means, float *vars, float *dgamma, float *dbeta, float *sums_out) {
    float *tmp = (float *)mid_malloc((size_t)R * 2 * C * sizeof(float));
    if (!tmp) return -3;
    int rc = finish(mid_bn_debug_merge(mi_global()->compute, R, C, means, vars, dgamma, dbeta, sums_out, tmp));
    mid_free(tmp);
    return rc;
}

/* the 3x3 convolutions of the bf16 path on channel-last zero-padded operands (kernels_cl_bf16.hip): operand re-laid, weights re-laid,
 * then the LDS-DMA kernel.  Same tensors and semantics as mi_op_conv_fwd_bf16 / mi_op_conv_dgrad_bf16 with k = 3.  -2: shape not covered */
int mi_op_conv_fwd_bf16_cl(const void *x, const float *w, void *y, int N, int C, int H, int K, int stride) {
    return op_conv(MID_BF16, MI_FWD_CL, OFF, OFF, x, w, NULL, y, NULL, N, C, H, K, 3, stride);
}
/* 1x1 forward with the input re-laid dense channel-last (one tap of the channel-last kernel: both operands reduction-contiguous) */
int mi_op_conv1x1_fwd_bf16_cl(const void *x, const float *w, void *y, int N, int C, int H, int K) {
    return op_conv(MID_BF16, MI_FWD_PW, OFF, OFF, x, w, NULL, y, NULL, N, C, H, K, 1, 1);
}
/* stride 1: dY re-laid as one zero-padded plane; stride 2: with a zero row / column at the far end (writes every element of dx: no addend) */
int mi_op_conv_dgrad_bf16_cl(const float *w, const void *dy, void *dx, int N, int C, int H, int K, int stride, int to_add) {
    if (stride == 2 && to_add) return -2;
    return op_conv(MID_BF16, OFF, stride == 2 ? MI_DG_CL2 : MI_DG_CL, OFF, NULL, w, dy, dx, to_add ? dx : NULL, N, C, H, K, 3, stride);
}
/* 3x3 weight gradient from the channel-last planes of BOTH operands (cl_wgrad2_kernel): stride 2 = the input's parity planes and the dY
 * planes of the stride-2 dgrad; stride 1 = both with a halo of 1 */
int mi_op_conv_wgrad_bf16_cl2(const void *x, const void *dy, float *dw, int N, int C, int H, int K, int stride) {
    return op_conv(MID_BF16, MI_FWD_CL, stride == 2 ? MI_DG_CL2 : MI_DG_CL, MI_WG_CL2, x, NULL, dy, dw, NULL, N, C, H, K, 3, stride);
}
/* ... and from the channel-last planes of the input and dY as it is (NCHW) */
int mi_op_conv_wgrad_bf16_cl(const void *x, const void *dy, float *dw, int N, int C, int H, int K, int stride) {
    return op_conv(MID_BF16, MI_FWD_CL, OFF, MI_WG_CL, x, NULL, dy, dw, NULL, N, C, H, K, 3, stride);
}
