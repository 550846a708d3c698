/*
 * layer.c -- everything that follows from one MiLayer alone (mi_host.h): the planner that gives a convolution its forward, dgrad and
 * wgrad kernel routes, names the kernel of each and sizes the buffers those kernels need, the allocation of exactly those buffers, the
 * layer's share of the workspaces, and the runners that re-lay operands and call the named kernel's launcher.  The trainer (trainer.c) keeps the network as
 * one table of units (MiUnit: a MiLayer with its batch norm, its tensors and the unit whose channel-last planes it writes), plans every
 * unit's layer with the planner's choices, and owns streams, events and the weight table.  The operator layer (ops.c) plans one layer
 * with forced routes and runs the same runners.  Plain C over mi_device.h.
 */
#include <stdio.h>
#include <string.h>
#include "mi_host.h"

void mi_layer_init(MiLayer *L, const float *w, int C, int H, int K, int k, int stride) {
    memset(L, 0, sizeof *L); /* MI_FWD_F32 / MI_DG_F32 / MI_WG_F32, no buffers */
    L->w = w; L->C = C; L->H = H; L->K = K; L->k = k; L->stride = stride;
}

/* ---------------------------------------------------------------------------------------------- */
/* The size limits of the routes ("Size limits"), for the shape a plan was refused: where a tensor is past one, the limit is
 * recorded (mi_last_error) -- a trainer or an operator at an unsupported batch then says why.  Returns 1 where it named a limit */
static int size_limit_named(const MiLayer *L, int dtype, int N, const int force[3]) {
    const int C = L->C, H = L->H, K = L->K, k = L->k, s = L->stride;
    if (N < 1 || C < 1 || H < 1 || K < 1 || k < 1 || s < 1) return 0;
    const int Ho = H / s;
    const double in = (double)N * C * H * H, out = (double)N * K * Ho * Ho;
    char msg[256];
    if ((double)N * H * H >= 2147483648.0) {
        snprintf(msg, sizeof msg, "size limit: a convolution takes fewer than 2^31 pixels per tensor (32-bit pixel indices); N = %d at %d x %d is %.0f", N, H, H, (double)N * H * H);
    } else if (dtype == MID_BF16 && k <= 3 && (in >= 2147480000.0 || out >= 2147480000.0)) {
        snprintf(msg, sizeof msg, "size limit: the bf16 convolutions take tensors of fewer than 2147480000 elements (32-bit byte offsets); N = %d gives %.0f in, %.0f out", N, in, out);
    } else if (dtype == MID_BF16 && k == 3 && force && (force[0] == MI_FWD_CL || force[1] == MI_DG_CL || force[1] == MI_DG_CL2) &&
               (double)N * (H + 2) * (H + 2) * (C > K ? C : K) * 2 >= 4294000000.0) {
        snprintf(msg, sizeof msg, "size limit: the channel-last bf16 routes take padded operands below 4294000000 bytes (32-bit byte offsets); N = %d is past it", N);
    } else return 0;
    mi_record_host_error("mi_layer_plan", msg);
    return 1;
}

/* The kernel of an MI_*_F32 route.  RESNET_MI_IGEMM (o->igemm) says which shapes may use the implicit GEMM at all: 0 none -- every
 * convolution on the older kernels; 1 the 1x1 weight gradients and the 3x3 / stride-2 projection shortcuts (K >= 2C) only -- the
 * bottleneck's own 3x3 convolutions stay on the direct VALU kernels, 1x1 forward / dgrad on gemm_mfma_kernel; 2 (default) every 3x3 and
 * 1x1.  Among those the kernel's own gate (shape, and tensors below 2^30 elements: so the batch decides too) has the last word; what it
 * leaves goes to the plain GEMM (1x1) or the direct kernels, whose launchers refuse the shapes nothing takes */
int mi_layer_f32_kernel(const MiOptions *o, int op, int N, int C, int H, int K, int k, int stride) {
    int ig = o->igemm != 0;
    if (k == 1 && op != 2 && o->igemm < 2) ig = 0;
    if (k == 3 && o->igemm == 1 && !(stride == 2 && K >= 2 * C && C >= 256)) ig = 0;
    if (ig && mi_igemm_supported(op, N, C, H, K, k, stride)) return MI_K_IGEMM;
    if (k == 1 && stride == 1) return MI_K_GEMM1X1;
    if (op != 2) return MI_K_DCONV;
    return mid_direct_wgradC_supported(N, C, H, K, k, stride) ? MI_K_WGRADC : MI_K_WGRAD;
}

static int layer_plan(MiLayer *L, int dtype, int policy, const MiOptions *o, int N, int site, const int force[3]);
int mi_layer_plan(MiLayer *L, int dtype, int policy, const MiOptions *o, int N, int site, const int force[3]) {
    /* every route indexes pixels (columns of the implicit GEMMs, rows of the direct kernels' patches) with 32 bits */
    if (N >= 1 && L->H >= 1 && (double)N * L->H * L->H >= 2147483648.0) { size_limit_named(L, dtype, N, force); return -2; }
    const int rc = layer_plan(L, dtype, policy, o, N, site, force);
    if (rc) size_limit_named(L, dtype, N, force);
    return rc;
}
static int layer_plan(MiLayer *L, int dtype, int policy, const MiOptions *o, int N, int site, const int force[3]) {
    const int C = L->C, H = L->H, K = L->K, k = L->k, s = L->stride;
    if ((dtype != MID_F32 && dtype != MID_BF16) || N < 1 || C < 1 || H < 1 || K < 1 || k < 1 || s < 1) return -2;
    /* the 7x7 stem keeps fp32 tensors and the fp32 kernels in every storage type, unless it runs on the matrix cores */
    const int bf = dtype == MID_BF16 && k <= 3;
    const int stem_mc = mid_stem_bf16_supported(C, H, K, k, s), k3 = bf && k == 3;
    L->N = N; L->dtype = dtype;
    L->cl_bytes = L->dye_bytes = L->par_bytes = L->xp_bytes = 0; L->scratch_floats = 0;

    int fwd = bf ? MI_FWD_BF16 : MI_FWD_F32;
    /* forward and weight gradient on one zero-padded channel-last plane (stride 1) or four channel-last parity planes (stride 2: the
     * striding convolutions are the spatial one and the projection) */
    if (k3 && (s == 1 ? o->cl_s1 : s == 2 && o->cl_s2) && mid_cl_supported(0, N, C, H, K, s)) fwd = MI_FWD_CL;
    /* fp32 storage: the stem in exact fp32 on the matrix cores (kernels_stem_bf16.hip, st32_*) */
    if (dtype == MID_F32 && o->igemm > 0 && stem_mc && o->stem_mfma) fwd = MI_FWD_STEM_F32;
    /* the stem on the bf16 matrix cores (image and weights rounded to bf16 like every other convolution of this mode) */
    if (dtype == MID_BF16 && stem_mc && o->bf16_stem) fwd = MI_FWD_STEM_BF16;
    if (force && force[0] != MI_PLANNED) fwd = force[0];
    switch (fwd) {
    case MI_NOT_RUN: L->kfwd = MI_K_NONE; break;
    case MI_FWD_F32: if (bf) return -2; L->kfwd = mi_layer_f32_kernel(o, 0, N, C, H, K, k, s); break;
    case MI_FWD_BF16: if (!bf || !mid_bf16_supported(0, N, C, H, K, k, s)) return -2; L->kfwd = MI_K_BGEMM; break;
    case MI_FWD_CL:
        if (!k3 || !mid_cl_supported(0, N, C, H, K, s)) return -2;
        L->cl_bytes = mid_cl_operand_bytes(0, N, C, H, K, s);
        L->kfwd = MI_K_CL_CONV;
        break;
    case MI_FWD_PW: /* one tap of the channel-last kernel on a dense channel-last input: both operands reduction-contiguous */
        if (!bf || k != 1 || s != 1 || !mid_cl_pw_supported(N, C, H, K)) return -2;
        L->cl_bytes = (size_t)N * H * H * C * 2 + 4096;
        L->kfwd = MI_K_CL_CONV;
        break;
    case MI_FWD_STEM_F32: case MI_FWD_STEM_BF16:
        if (!stem_mc) return -2;
        L->xp_bytes = fwd == MI_FWD_STEM_F32 ? mid_stem_f32_xp_bytes(N, H) : mid_stem_bf16_xp_bytes(N, H);
        L->scratch_floats = mid_stem_bf16_part_floats(N, H);
        L->kfwd = fwd == MI_FWD_STEM_F32 ? MI_K_ST32_FWD : MI_K_ST_FWD;
        break;
    default: return -2;
    }
    /* the bf16 stem's output and that tensor's gradient are stored as bf16 like every other convolution's (they stay in their
     * fp32-sized buffers): 822 MB tensors at N = 256 that the stem BN reads twice forward and three times backward */
    L->out_dt = bf || (fwd == MI_FWD_STEM_BF16 && dtype == MID_BF16 && !o->stem_tensors_f32) ? MID_BF16 : MID_F32;

    int dgrad = bf ? MI_DG_BF16 : MI_DG_F32;
    /* the dgrad on dY re-laid as one zero-padded plane (stride 1, beside a channel-last forward), or with a zero row / column at the
     * far end (stride 2) */
    if (k3 && s == 1 && fwd == MI_FWD_CL && o->cl_s1_dgrad && mid_cl_supported(1, N, C, H, K, 1)) dgrad = MI_DG_CL;
    if (k3 && s == 2 && o->cl_dgrad2 && mid_cl_dgrad2_supported(N, C, H, K)) dgrad = MI_DG_CL2;
    if (force && force[1] != MI_PLANNED) dgrad = force[1];
    switch (dgrad) {
    case MI_NOT_RUN: L->kdgrad = MI_K_NONE; break;
    case MI_DG_F32: if (bf) return -2; L->kdgrad = mi_layer_f32_kernel(o, 1, N, C, H, K, k, s); break;
    case MI_DG_BF16: if (!bf || !mid_bf16_supported(1, N, C, H, K, k, s)) return -2; L->kdgrad = MI_K_BGEMM; break;
    case MI_DG_CL:
        if (!k3 || s != 1 || !mid_cl_supported(1, N, C, H, K, 1)) return -2;
        L->dye_bytes = mid_cl_operand_bytes(1, N, C, H, K, 1);
        L->kdgrad = MI_K_CL_CONV;
        break;
    case MI_DG_CL2:
        if (!k3 || s != 2 || !mid_cl_dgrad2_supported(N, C, H, K)) return -2;
        L->dye_bytes = mid_cl_dgrad2_operand_bytes(N, K, H / 2);
        L->kdgrad = MI_K_CL_DGRAD2;
        break;
    default: return -2;
    }

    const int P = (H / s) * (H / s);
    const int wg = fwd == MI_FWD_CL && mid_cl_wgrad_supported(N, C, H, K, s), wg2 = fwd == MI_FWD_CL && mid_cl_wgrad2_supported(N, C, H, K, s);
    int wgrad = bf ? MI_WG_BF16 : MI_WG_F32;
    /* both operands channel-last (the dY planes of the dgrad) where the plane does not fill 64-pixel tiles (784, 196, 49 pixels: all
     * of the benchmark network's stride-2 layers; -0.8 ms per step, most of it the two 7x7 layers the other kernel cannot take) */
    if (L->dye_bytes && wg2 && (P % 64 != 0 || !wg)) wgrad = MI_WG_CL2;
    else if (wg) wgrad = MI_WG_CL;
    if (fwd == MI_FWD_STEM_F32) wgrad = MI_WG_STEM_F32; /* (the weight gradient reads the planes the forward left) */
    if (fwd == MI_FWD_STEM_BF16) wgrad = MI_WG_STEM_BF16;
    if (force && force[2] != MI_PLANNED) wgrad = force[2];
    switch (wgrad) {
    case MI_NOT_RUN: L->kwgrad = MI_K_NONE; break;
    case MI_WG_F32: if (bf) return -2; L->kwgrad = mi_layer_f32_kernel(o, 2, N, C, H, K, k, s); break;
    case MI_WG_BF16: /* 1x1: both operands staged as they lie by LDS-DMA (kernels_cl_bf16.hip), where the shape tiles */
        if (!bf || !mid_bf16_supported(2, N, C, H, K, k, s)) return -2;
        L->kwgrad = k == 1 && s == 1 && o->pw_wgrad && mid_pw_wgrad_supported(N, C, H, K) ? MI_K_PW_WGRAD : MI_K_BGEMM;
        break;
    case MI_WG_CL: if (!wg) return -2; L->kwgrad = MI_K_CL_WGRAD; break;
    case MI_WG_CL2: if (!wg2 || !L->dye_bytes) return -2; L->kwgrad = MI_K_CL_WGRAD2; break;
    case MI_WG_STEM_F32: if (fwd != MI_FWD_STEM_F32) return -2; L->kwgrad = MI_K_ST32_WGRAD; break;
    case MI_WG_STEM_BF16: if (fwd != MI_FWD_STEM_BF16) return -2; L->kwgrad = MI_K_ST_WGRAD; break;
    default: return -2;
    }
    /* NCHW parity planes of a stride-2 input (kernels_igemm_bf16.hip): the NCHW forward writes them and the weight gradient reads
     * them again (1.1 GB in all at N = 256 with every stride-2 layer on this route); behind a channel-last forward, only for
     * shapes that no channel-last weight-gradient kernel takes (the NCHW one makes them itself) */
    if (s == 2 && (fwd == MI_FWD_BF16 || (wgrad == MI_WG_BF16 && !wg2))) L->par_bytes = (size_t)N * C * H * H * 2;
    L->fwd = fwd; L->dgrad = dgrad; L->wgrad = wgrad;

    /* the forms a weight table re-lays once per forward pass (mid_conv_prelayout_all): every bf16 convolution (k-step tiles, forward
     * and dgrad forms), the fp32 ones on the implicit GEMM (RESNET_MI_PRELAYOUT=0: each re-lays its own; its 1x1 dgrad reads the KC
     * tensor as it is) */
    L->wre_fwd = bf || (o->prelayout && L->kfwd == MI_K_IGEMM);
    L->wre_dgrad = bf || (o->prelayout && L->kdgrad == MI_K_IGEMM && k == 3);
    L->wre_floats = ((size_t)k * k * C * K) / (bf ? 2 : 1);

    /* The dgrad also does the reduction pass of the BN' its output feeds (and gates that output): sites 1 expansion dgrad -> spatial
     * BN', 2 spatial dgrad -> reduction BN', 4 reduction dgrad -> the expansion BN' of the identity block below.  bf16: every site
     * whose dgrad is on the NCHW kernel (RECOMPUTE_BN too: the gating tensors have just been re-derived when the dgrad runs).
     * fp32: the sites of RESNET_MI_F32_BNFUSE_BWD where every tiling shape is on the implicit GEMM, not with the FULL policy (its derivative mirror keeps
     * the ungated gradients the dump tree names).  Measured at batch 256 (same box, ms/step): none 108.3-109.5, site 4 alone
     * 108.3-108.9, site 1 alone 109.4-110.2, sites 1+2 111.6-112.8, all 111.7-112.2 -- the fp32 epilogue keeps lane = column, so
     * the fused form reads x / mask / addend with 4-byte accesses (four times the memory instructions of the bf16 kernel's
     * row-major drain) and pays for it wherever the separate reduction pass was only 2 tensors; site 4 replaces a 4-tensor pass
     * and breaks even, so it is the default. */
    const int f32_sites = o->igemm >= 2 ? o->bnfuse_bwd_f32 : 0;
    L->fz = site && o->bnfuse_bwd &&
            (dgrad == MI_DG_BF16 || (dgrad == MI_DG_F32 && (f32_sites & site) && policy != MI_STORE_FULL));
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* guard: MI_GUARD bytes of slack on both sides (see mi_malloc); zero: the buffer starts zeroed -- the halos of the channel-last
 * planes stay zero, their writers fill the interior only */
static void *lalloc(MiCtx *c, size_t bytes, int guard, int zero) {
    if (!bytes) return NULL;
    char *p = (char *)mi_ctx_alloc(c, bytes + (guard ? 2 * MI_GUARD : 0));
    if (zero) mid_memset(p, 0, bytes, mi_global()->compute);
    return guard ? p + MI_GUARD : p;
}
static int xp_guard(const MiLayer *L) { return L->fwd == MI_FWD_STEM_BF16; } /* (bf16 planes; the fp32 planes are read whole) */
void mi_layer_alloc(MiCtx *c, MiLayer *L) {
    L->cl = lalloc(c, L->cl_bytes, 0, L->fwd == MI_FWD_CL);
    L->dye = lalloc(c, L->dye_bytes, 0, 1);
    L->par = lalloc(c, L->par_bytes, 1, 0);
    L->xp = lalloc(c, (L->xp_bytes + 3) / 4 * 4, xp_guard(L), 0);
    L->scratch = (float *)lalloc(c, L->scratch_floats * sizeof(float), 0, 0);
    L->par_valid = 0;
}
void mi_layer_free(MiLayer *L) {
    mid_free(L->cl); mid_free(L->dye); mid_free(L->scratch);
    if (L->par) mid_free((char *)L->par - MI_GUARD);
    if (L->xp) mid_free((char *)L->xp - (xp_guard(L) ? MI_GUARD : 0));
    if (L->we) { mid_free(L->we->fwd); mid_free(L->we->dgrad); }
    L->cl = L->dye = L->par = L->xp = NULL; L->scratch = NULL; L->we = NULL;
}
int mi_layer_own_weights(MiLayer *L, mid_wt_entry *e, mid_stream s) {
    int rc = 0;
    memset(e, 0, sizeof *e);
    L->we = e;
    if (L->fwd == MI_FWD_CL || L->fwd == MI_FWD_PW) {
        e->fwd = (float *)lalloc(NULL, L->wre_floats * sizeof(float), 0, 0);
        rc = mid_bf16_prelayout_fwd(s, L->w, e->fwd, L->K, L->C, L->k);
    }
    if (!rc && (L->dgrad == MI_DG_CL || L->dgrad == MI_DG_CL2)) {
        e->dgrad = (float *)lalloc(NULL, L->wre_floats * sizeof(float), 0, 0);
        rc = mid_bf16_prelayout_dgrad(s, L->w, e->dgrad, L->K, L->C, L->k);
    }
    return rc;
}

/* the workspaces every convolution of a table shares, sized for its largest layer */
void mi_layer_need(const MiLayer *L, MiLayerNeed *need) {
    const int N = L->N, C = L->C, H = L->H, K = L->K, k = L->k, s = L->stride;
    /* re-laid weights; behind them the partial tiles of the implicit GEMM's sliced tail round */
    size_t a = mid_conv_ws_wt_floats(C, K, k) + (L->kfwd == MI_K_IGEMM || L->kdgrad == MI_K_IGEMM ? mi_igemm_tail_floats() : 0), b = 0, e;
    switch (L->kwgrad) { /* the split partials of the weight gradient */
    case MI_K_IGEMM: b = mi_igemm_part_floats(N, C, H, K, k, s); break;
    case MI_K_GEMM1X1: b = mi_conv1x1_wgrad_part_floats(N, C, H * H, K); break;
    case MI_K_WGRADC: b = mid_direct_wgradC_part_floats(N, C, H, K, k, s); break;
    case MI_K_WGRAD: b = mid_direct_wgrad_part_floats(N, C, H, K, k, s); break;
    case MI_K_BGEMM: b = mi_bgemm_part_floats(N, C, H, K, k, s); break;
    case MI_K_PW_WGRAD: b = mid_pw_wgrad_part_floats(N, C, H, K); break;
    case MI_K_CL_WGRAD: b = mid_cl_wgrad_part_floats(N, C, H, K, s); break;
    case MI_K_CL_WGRAD2: b = mid_cl_wgrad2_part_floats(N, C, H, K, s); break;
    default: break; /* (the stem's partials are the layer's own scratch) */
    }
    if (a > need->wt) need->wt = a;
    if (b > need->part) need->part = b;
    /* the statistics partials of the layer's own output; a fusing dgrad leaves the sums of the BN' below in the same table */
    if ((e = mid_bn_parts_floats(N, K, H / s)) > need->bn_parts) need->bn_parts = e;
    if (L->fz && (e = mid_bn_parts_floats(N, C, H)) > need->bn_parts) need->bn_parts = e;
    if (K > need->maxc) need->maxc = K;
    if (C > need->maxc) need->maxc = C;
}
void mi_layer_ws_alloc(MiCtx *c, MiLayerWs *w, const MiLayerNeed *need) {
    memset(w, 0, sizeof *w);
    w->ws.wt_floats = need->wt; w->ws.part_floats = need->part;
    w->ws.wt = (float *)lalloc(c, need->wt * sizeof(float), 0, 0);
    w->ws.part = (float *)lalloc(c, need->part * sizeof(float), 0, 0);
    w->bn_ws = (float *)lalloc(c, mid_bn_ws_floats(need->maxc) * sizeof(float), 0, 0);
    w->bn_parts.floats = need->bn_parts;
    w->bn_parts.buf = (float *)lalloc(c, need->bn_parts * sizeof(float), 0, 0);
}
void mi_layer_ws_free(MiLayerWs *w) {
    mid_free(w->ws.wt); mid_free(w->ws.part); mid_free(w->bn_ws); mid_free(w->bn_parts.buf);
    memset(w, 0, sizeof *w);
}

/* ---------------------------------------------------------------------------------------------- */
int mi_layer_x_relayout(const MiLayer *L, mid_stream s, const void *x) {
    if (L->fwd == MI_FWD_PW) return mid_cl_relayout_dense(s, x, L->cl, L->N, L->C, L->H);
    return mid_cl_relayout(s, x, L->cl, L->N, L->C, L->H, L->stride == 2);
}
int mi_layer_fwd(MiLayer *L, MiLayerWs *w, mid_stream s, const void *x, void *y, mid_bn_parts *parts) {
    const int N = L->N, C = L->C, H = L->H, K = L->K;
    int rc = 0;
    w->ws.s2d = L->par; w->ws.s2d_bytes = L->par_bytes; w->ws.s2d_valid = 0;
    w->ws.pre_fwd = L->we ? L->we->fwd : NULL; /* re-laid at the start of this forward pass */
    switch (L->fwd) {
    case MI_FWD_STEM_F32:
        rc = mid_stem_fwd_f32(s, (const float *)x, L->w, (float *)y, L->xp, L->xp_bytes, L->scratch, L->scratch_floats, N, H, parts);
        break;
    case MI_FWD_STEM_BF16: /* (the stem's tensors may be fp32 here, but its statistics still come from the kernel's accumulators) */
        rc = mid_stem_fwd_bf16(s, (const float *)x, L->w, y, L->out_dt, L->xp, L->xp_bytes, L->scratch, L->scratch_floats, N, H, parts);
        break;
    case MI_FWD_CL: /* planes written by the producing BN apply, else re-laid here; the weight gradient reads them again */
        if (!L->cl_by_bn) rc = mi_layer_x_relayout(L, s, x);
        if (!rc) rc = mid_cl_fwd(s, L->cl, L->we->fwd, y, N, C, H, K, L->stride, parts);
        L->par_valid = 0;
        break;
    case MI_FWD_PW:
        rc = mi_layer_x_relayout(L, s, x);
        if (!rc) rc = mid_cl_pw_fwd(s, L->cl, L->we->fwd, y, N, C, H, K, parts);
        break;
    case MI_FWD_BF16:
        rc = mid_conv_fwd_bf16(s, &w->ws, x, L->w, y, N, C, H, K, L->k, L->stride, parts);
        L->par_valid = w->ws.s2d_valid; /* the launch says whether it left the parity planes */
        break;
    default: /* MI_FWD_F32; only the implicit GEMM leaves statistics partials */
        if (parts) parts->nparts = 0;
        if (L->kfwd == MI_K_IGEMM) rc = mi_igemm_fwd(s, &w->ws, (const float *)x, L->w, (float *)y, N, C, H, K, L->k, L->stride, parts);
        else if (L->kfwd == MI_K_GEMM1X1) rc = mi_conv1x1_fwd(s, (const float *)x, L->w, (float *)y, N, C, H * H, K);
        else rc = mid_direct_fwd(s, &w->ws, (const float *)x, L->w, (float *)y, N, C, H, K, L->k, L->stride);
    }
    w->ws.pre_fwd = NULL;
    return rc;
}
/* the batch norm (+ReLU | +residual+ReLU) behind the convolution.  cl_reader: a convolution this unit's output feeds; where its
 * channel-last input planes are this BN's to write (cl_by_bn), the BN apply writes them beside its NCHW output */
int mi_layer_bn_fwd(const MiLayer *L, MiLayerWs *w, mid_stream s, const mid_bn_parts *parts, const void *conv_out, const float *gamma,
                    const float *beta, const void *residual, float *means, float *vars, void *y, float *xhat_out, float *norm_out, float eps,
                    int relu, const MiLayer *cl_reader) {
    const int Ho = L->H / L->stride;
    void *ycl = cl_reader && cl_reader->cl_by_bn ? cl_reader->cl : NULL;
    const int Hcl = ycl ? (cl_reader->stride == 2 ? -cl_reader->H : cl_reader->H) : 0;
    return mid_bn_fwd_t(s, w->bn_ws, parts, conv_out, L->out_dt, gamma, beta, residual, means, vars, y, L->dtype, xhat_out, norm_out, L->N,
                        L->K, Ho * Ho, eps, relu, ycl, Hcl);
}
/* the same apply with GIVEN statistics (the eval pass: a layer's running means / variances): the kernel, the storage types and the
 * channel-last side output of mi_layer_bn_fwd, no reduction, means / vars only read */
int mi_layer_bn_apply(const MiLayer *L, mid_stream s, const void *conv_out, const float *gamma, const float *beta, const void *residual,
                      const float *means, const float *vars, void *y, float eps, int relu, const MiLayer *cl_reader) {
    const int Ho = L->H / L->stride;
    void *ycl = cl_reader && cl_reader->cl_by_bn ? cl_reader->cl : NULL;
    const int Hcl = ycl ? (cl_reader->stride == 2 ? -cl_reader->H : cl_reader->H) : 0;
    return mid_bn_apply_t(s, conv_out, L->out_dt, gamma, beta, residual, means, vars, y, L->dtype, L->N, L->K, Ho * Ho, eps, relu, ycl, Hcl);
}

/* the channel-last copy of dy that the channel-last dgrad AND the weight gradient read */
int mi_layer_dy_relayout(const MiLayer *L, mid_stream s, const void *dy) {
    const int Ho = L->H / L->stride;
    if (L->dgrad == MI_DG_CL) return mid_cl_relayout(s, dy, L->dye, L->N, L->K, Ho, 0); /* stride 1: one plane with a halo of 1 */
    if (L->dgrad == MI_DG_CL2) return mid_cl_relayout_end(s, dy, L->dye, L->N, L->K, Ho); /* stride 2: a zero row / column at the far end */
    return 0;
}
/* the request for a fusing dgrad (L->fz): the reduction over x / mask / means of the BN' its output feeds; NULL where L does not fuse */
const mid_bn_bwd_parts *mi_layer_fz_request(const MiLayer *L, const MiLayerWs *w, mid_bn_bwd_parts *r, const void *x, const void *mask,
                                            const float *means) {
    if (!L->fz) return NULL;
    r->x = x; r->mask = mask; r->means = means;
    r->buf = w->bn_parts.buf; r->floats = w->bn_parts.floats; r->nparts = 0;
    return r;
}
/* req (mi_layer_fz_request): the dgrad also does the reduction pass of the BN' its output feeds; it hands that over in *fz (nparts > 0
 * when the launch could do it, dx then holds the gated gradient; fp32: the implicit GEMM at stride 1 can, every other kernel runs the
 * plain dgrad and hands back nparts = 0) */
int mi_layer_dgrad(const MiLayer *L, MiLayerWs *w, mid_stream s, const void *dy, void *dx, const void *addend, const mid_bn_bwd_parts *req,
                   mid_bn_bwd_parts *fz) {
    const int N = L->N, C = L->C, H = L->H, K = L->K, k = L->k, st = L->stride;
    int rc;
    /* stride 1 on the channel-last dY plane (the BN' below then runs its own reduction pass: measured neutral) */
    if (L->dgrad == MI_DG_CL) return mid_cl_dgrad(s, L->dye, L->we->dgrad, dx, addend, N, C, H, K);
    /* stride 2 on the channel-last dY: both column parities of dx per workgroup by LDS-DMA staged MFMAs (dense stores; 1.5-1.9x
     * the NCHW kernel's four parity classes).  It writes every element of dx: no addend (the stride-2 layers' dgrads have none) */
    if (L->dgrad == MI_DG_CL2) return mid_cl_dgrad2(s, L->dye, L->we->dgrad, dx, N, C, H, K);
    w->ws.pre_dgrad = L->we ? L->we->dgrad : NULL;
    if (req) { *fz = *req; fz->nparts = 0; }
    if (L->dgrad == MI_DG_BF16 && req) rc = mid_conv_dgrad_bn_bf16(s, &w->ws, L->w, dy, dx, addend, N, C, H, K, k, st, fz);
    else if (L->dgrad == MI_DG_BF16) rc = mid_conv_dgrad_bf16(s, &w->ws, L->w, dy, dx, addend, N, C, H, K, k, st);
    else if (L->kdgrad == MI_K_IGEMM)
        rc = mi_igemm_dgrad(s, &w->ws, L->w, (const float *)dy, (float *)dx, (const float *)addend, N, C, H, K, k, st, req && st == 1 ? fz : NULL);
    else if (L->kdgrad == MI_K_GEMM1X1) rc = mi_conv1x1_dgrad(s, L->w, (const float *)dy, (float *)dx, (const float *)addend, N, C, H * H, K);
    else rc = mid_direct_dgrad(s, &w->ws, L->w, (const float *)dy, (float *)dx, (const float *)addend, N, C, H, K, k, st);
    w->ws.pre_dgrad = NULL;
    return rc;
}
int mi_layer_wgrad(const MiLayer *L, MiLayerWs *w, mid_stream s, const void *x, const void *dy, float *dw) {
    const int N = L->N, C = L->C, H = L->H, K = L->K, k = L->k, st = L->stride;
    /* the forward pass left the parity planes of x in the layer's own buffer: the weight gradient reads them again */
    w->ws.s2d = L->par; w->ws.s2d_bytes = L->par_bytes; w->ws.s2d_valid = L->par && L->par_valid;
    switch (L->wgrad) {
    case MI_WG_STEM_F32: return mid_stem_wgrad_f32(s, L->xp, (const float *)dy, dw, L->scratch, L->scratch_floats, N, H);
    case MI_WG_STEM_BF16: /* the forward pass left the batch as padded bf16 parity planes */
        return mid_stem_wgrad_bf16(s, L->xp, dy, L->out_dt, dw, L->scratch, L->scratch_floats, N, H);
    case MI_WG_CL2: /* both operands channel-last: the forward's input planes and the dY planes mi_layer_dy_relayout has made */
        return mid_cl_wgrad2(s, L->cl, L->dye, dw, w->ws.part, w->ws.part_floats, N, C, H, K, st);
    case MI_WG_CL: return mid_cl_wgrad(s, L->cl, dy, dw, w->ws.part, w->ws.part_floats, N, C, H, K, st);
    case MI_WG_BF16:
        if (L->kwgrad == MI_K_PW_WGRAD) return mid_pw_wgrad(s, x, dy, dw, w->ws.part, w->ws.part_floats, N, C, H, K);
        return mi_bgemm_wgrad(s, &w->ws, x, dy, dw, N, C, H, K, k, st);
    default: break; /* MI_WG_F32 */
    }
    switch (L->kwgrad) {
    case MI_K_IGEMM: return mi_igemm_wgrad(s, &w->ws, (const float *)x, (const float *)dy, dw, N, C, H, K, k, st);
    case MI_K_GEMM1X1: return mi_conv1x1_wgrad(s, &w->ws, (const float *)x, (const float *)dy, dw, N, C, H * H, K);
    case MI_K_WGRADC: return mid_direct_wgradC(s, &w->ws, (const float *)x, (const float *)dy, dw, N, C, H, K, k, st);
    default: return mid_direct_wgrad(s, &w->ws, (const float *)x, (const float *)dy, dw, N, C, H, K, k, st);
    }
}
/* BN' (+fused ReLU') of a unit of C channels over P pixels.  fz: the hand-off of the dgrad that produced dy -- nparts > 0: it gated dy
 * and left the sums (merge, finalize, apply; the hand-off is taken); else the whole backward, mask_mode 3: ReLU' of mask_src fused in
 * and its product with dy kept (gated_out) */
int mi_bn_bwd_unit(MiLayerWs *w, mid_stream s, mid_bn_bwd_parts *fz, const void *x, int x_dt, const float *gamma, const float *beta,
                   const float *means, const float *vars, const void *dy, const void *mask_src, int mask_mode, void *gated_out, int a_dt,
                   void *dx, float *dgamma, float *dbeta, int N, int C, int P, float eps) {
    if (fz->nparts <= 0)
        return mid_bn_bwd_t(s, w->bn_ws, x, x_dt, gamma, beta, means, vars, dy, mask_src, gated_out, a_dt, dx, dgamma, dbeta, N, C, P, eps, mask_mode);
    const int rc = mid_bn_bwd_parts_t(s, w->bn_ws, fz, x, x_dt, gamma, beta, means, vars, dy, a_dt, dx, dgamma, dbeta, N, C, P, eps);
    fz->nparts = 0;
    return rc;
}

/* ---------------------------------------------------------------------------------------------- */
static int planned(MiLayer *L, int dtype, int policy, int N, int C, int H, int K, int k, int stride, int site) {
    MiOptions o;
    if (policy < MI_STORE_FAST || policy > MI_STORE_FULL || (site != 0 && site != 1 && site != 2 && site != 4)) return -2;
    mi_read_options(&o);
    mi_layer_init(L, NULL, C, H, K, k, stride);
    return mi_layer_plan(L, dtype, policy, &o, N, site, NULL) ? -2 : 0;
}
int mi_layer_routes(int dtype, int policy, int N, int C, int H, int K, int k, int stride, int site, int out[4]) {
    MiLayer L;
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (planned(&L, dtype, policy, N, C, H, K, k, stride, site)) return -2;
    out[0] = L.fwd; out[1] = L.dgrad; out[2] = L.wgrad; out[3] = L.fz;
    return 0;
}
int mi_layer_kernels(int dtype, int policy, int N, int C, int H, int K, int k, int stride, int site, int out[3]) {
    MiLayer L;
    for (int i = 0; i < 3; i++) out[i] = 0;
    if (planned(&L, dtype, policy, N, C, H, K, k, stride, site)) return -2;
    out[0] = L.kfwd; out[1] = L.kdgrad; out[2] = L.kwgrad;
    return 0;
}
