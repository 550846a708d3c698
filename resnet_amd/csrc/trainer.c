/*
 * trainer.c -- host side of the drop-in trainer surface, in C over the thin device header (mi_device.h).
 * Mirrors the reference's L3/L4 layers: init_dimensions / init_resnet / init_trainer (resnet.cu:666-1194),
 * forward_pass (resnet.cu:1526-1775), backwards_pass (resnet.cu:1777-2248 with the spatial-BN fix of
 * resnet_cudnn.cu:2365-2366), update_parameters (resnet.cu:2910-2987).
 *
 * What is deliberately different from the reference (same results, MI355X-first structure):
 *  - one stream-ordered launch sequence, no cudaMalloc/cudaFree or blocking copies inside a step
 *    (the reference mallocs in FC backward, resnet.cu:1484-1508, and leaks in :2080);
 *  - parameters / gradients / Adam moments live in four contiguous arenas with identical offsets, so the
 *    480 Adam launches + 160 memsets + per-tensor D2H NaN scans of resnet.cu:2952-2978 are one launch, one
 *    memset and one 4-byte flag, and the gradient all-reduce runs over contiguous buckets;
 *  - BN stores only what backward needs (conv output, mean, var, activated); x-hat / BN-out / pre-ReLU
 *    sums exist only in full-store mode; BN+residual-add+ReLU is one kernel; ReLU' is fused into BN';
 *  - activation derivatives use six rolling buffers (the policy of resnet_cudnn_lowmem.cu:2152-2170)
 *    instead of a full mirror of the activation tree (resnet.cu:1151).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_host.h"

static MiGlobal G;
MiGlobal *mi_global(void) {
    if (!G.ready) {
        G.compute = mid_stream_create();
        G.comm = mid_stream_create();
        G.copy = mid_stream_create();
        G.aux = mid_stream_create_low_priority();
        G.ready = 1;
    }
    return &G;
}

int mi_device_count(void) { return mid_device_count(); }
int mi_set_device(int device) { return mid_set_device(device); }
const char *mi_last_error(void) { return mid_last_error(); }
void mi_device_synchronize(void) { mid_device_sync(); }
/* Any host write into device memory may have been a parameter (weight injection, resume).  mi_copy_to_device knows no trainer,
 * so it advances a process-wide write counter; every trainer remembers the count its re-laid weight copies were made at
 * (MiCtx.host_epoch_seen) and its own "Adam ran since" flag (MiCtx.params_dirty): staleness is per trainer, two trainers in one
 * process cannot clear each other's. */
static unsigned long g_host_write_epoch = 0;
void mi_params_mark_dirty(void) { g_host_write_epoch++; }
void mi_copy_to_device(void *d, const void *s, size_t n) { MiGlobal *g = mi_global(); mid_memcpy_h2d(d, s, n, g->compute); mid_stream_sync(g->compute); g_host_write_epoch++; }
void mi_copy_to_host(void *d, const void *s, size_t n) { MiGlobal *g = mi_global(); mid_memcpy_d2h(d, s, n, g->compute); mid_stream_sync(g->compute); }

void mi_prof_enable(int on) { mid_prof_enable(on); }
void mi_prof_reset(void) { mid_prof_reset(); }
void mi_prof_get(int family, long *launches, double *ms, double *flops, double *bytes) { mid_prof_get(family, launches, ms, flops, bytes); }

MiRng *mi_rng_create(uint64_t seed) {
    MiRng *r = (MiRng *)calloc(1, sizeof(MiRng));
    r->seed = seed;
    return r;
}
void mi_rng_destroy(MiRng *r) { free(r); }

void *mi_ctx_alloc(MiCtx *c, size_t bytes) {
    void *p = mid_malloc(bytes);
    if (!p) { fprintf(stderr, "resnet_mi: device allocation of %zu bytes failed: %s\n", bytes, mid_last_error()); exit(1); }
    if (c) {
        if (c->n_allocs == c->cap_allocs) {
            c->cap_allocs = c->cap_allocs ? c->cap_allocs * 2 : 256;
            c->allocs = (void **)realloc(c->allocs, sizeof(void *) * c->cap_allocs);
            c->alloc_bytes = (size_t *)realloc(c->alloc_bytes, sizeof(size_t) * c->cap_allocs);
        }
        c->alloc_bytes[c->n_allocs] = bytes;
        c->allocs[c->n_allocs++] = p;
        c->dev_bytes += bytes;
        if (c->counting_act) c->act_bytes += bytes;
    }
    return p;
}
/* frees allocs[first ..): everything a rebuild of the activation buffers replaces */
static void ctx_free_from(MiCtx *c, int first) {
    for (int i = first; i < c->n_allocs; i++) { mid_free(c->allocs[i]); c->dev_bytes -= c->alloc_bytes[i]; }
    c->n_allocs = first;
}
/* every live trainer context: a rank that is about to exit on an error tears ALL its communicators down first (gradient
 * buckets and sync-BN), so that its peers' collectives fail instead of hanging */
static MiCtx *g_live = NULL;
static void abort_all_comms(void) {
    for (MiCtx *c = g_live; c; c = c->next_live) {
        if (c->comm) { mid_rccl_comm_abort(c->comm); c->comm = NULL; }
        if (c->sync_bn_comm) { mid_bn_set_sync(NULL, 1, NULL, 0, 0); mid_rccl_comm_abort(c->sync_bn_comm); c->sync_bn_comm = NULL; }
    }
}
/* a launcher that fails leaves unwritten tensors behind: stop like the allocation failure does (the reference's void
 * API gives its caller nothing to poll) */
static void ck(int rc, const char *what) {
    if (rc) { fprintf(stderr, "resnet_mi: %s failed (%d): %s\n", what, rc, mid_last_error()); abort_all_comms(); exit(1); }
}

/* resnet.cu:666-682 */
Dims *init_dimensions(int input, int init_kernel_dim, int init_conv_filters, int init_conv_stride, int init_maxpool_dim,
                      int init_maxpool_stride, int n_conv_blocks, int *is_block_spatial_reduction, int final_depth,
                      int output) {
    Dims *d = (Dims *)malloc(sizeof(Dims));
    d->input = input; d->init_kernel_dim = init_kernel_dim; d->init_conv_filters = init_conv_filters;
    d->init_conv_stride = init_conv_stride; d->init_maxpool_dim = init_maxpool_dim;
    d->init_maxpool_stride = init_maxpool_stride; d->n_conv_blocks = n_conv_blocks;
    d->is_block_spatial_reduction = is_block_spatial_reduction; d->final_depth = final_depth; d->output = output;
    return d;
}

/* ---------------------------------------------------------------------------------------------- */
/* Parameter-shaped structure over one contiguous arena.  Location order = resnet.cu:838-943.       */
#define ARENA_ALIGN 64
static size_t align_up(size_t v) { return (v + ARENA_ALIGN - 1) / ARENA_ALIGN * ARENA_ALIGN; }

typedef struct { float *base; size_t off; float **loc; int *sizes; int n; double *var; } Carver;
static float *carve(Carver *c, int size, double var /* <0: gamma, ==0: zero */) {
    float *p = c->base + c->off;
    c->loc[c->n] = p; c->sizes[c->n] = size; c->var[c->n] = var; c->n++;
    c->off += align_up((size_t)size);
    return p;
}
static BatchNorm *make_bn(Carver *c, int spatial, int depth) {
    BatchNorm *b = (BatchNorm *)malloc(sizeof(BatchNorm));
    b->spatial_dim = spatial; b->depth = depth;
    b->gamma = carve(c, depth, -1.0);
    b->beta = carve(c, depth, 0.0);
    return b;
}
static int count_locations(const Dims *d, size_t *arena) {
    int n = 3, inc = d->init_conv_filters, ex = 4 * inc, red = inc;
    size_t a = align_up((size_t)d->init_kernel_dim * d->init_kernel_dim * inc * 3) + 2 * align_up(inc);
    for (int i = 0; i < d->n_conv_blocks; i++) {
        int stride = 1;
        if (d->is_block_spatial_reduction[i] == 1) { stride = 2; red *= 2; ex *= 2; }
        n += 9;
        a += align_up((size_t)inc * red) + align_up((size_t)red * red * 9) + align_up((size_t)ex * red) + 4 * align_up(red) + 2 * align_up(ex);
        if (inc != ex) { n += 3; a += align_up((size_t)inc * ex * (stride == 2 ? 9 : 1)) + 2 * align_up(ex); }
        inc = ex;
    }
    n += 1;
    a += align_up((size_t)ex * d->output);
    *arena = a;
    return n;
}
size_t mi_params_arena_floats(const Params *p) {
    const int l = p->n_locations - 1;
    return (size_t)(p->locations[l] - p->locations[0]) + align_up((size_t)p->sizes[l]);
}
float *mi_params_arena_base(const Params *p) { return p->locations[0]; }

/* init_model_parameters, resnet.cu:805-949.  gen == NULL -> zero twin (gradients, Adam moments, :1148-1150) */
static Params *build_params(const Dims *d, MiRng *gen, MiCtx *owner) {
    size_t arena_floats;
    const int nloc = count_locations(d, &arena_floats);
    Params *p = (Params *)malloc(sizeof(Params));
    Carver c;
    c.base = (float *)mi_ctx_alloc(owner, arena_floats * sizeof(float));
    c.off = 0; c.n = 0;
    c.loc = (float **)malloc(sizeof(float *) * nloc);
    c.sizes = (int *)malloc(sizeof(int) * nloc);
    c.var = (double *)malloc(sizeof(double) * nloc);
    const int f = d->init_conv_filters, kd = d->init_kernel_dim;
    p->init_conv_layer = carve(&c, kd * kd * f * 3, 2.0 / (7.0 * 7.0 * (3 + f))); /* fan literal 7*7, resnet.cu:831 */
    p->norm_init_conv = make_bn(&c, d->input / d->init_conv_stride, f);
    p->conv_blocks = (ConvBlock **)malloc(sizeof(ConvBlock *) * (d->n_conv_blocks > 0 ? d->n_conv_blocks : 1));
    int inc = f, H = d->input / 4, red = f, ex = 4 * f; /* resnet.cu:857-862 */
    for (int i = 0; i < d->n_conv_blocks; i++) {
        int stride = 1;
        if (d->is_block_spatial_reduction[i] == 1) { stride = 2; red *= 2; ex *= 2; }
        ConvBlock *b = (ConvBlock *)calloc(1, sizeof(ConvBlock));
        b->incoming_filters = inc; b->incoming_spatial_dim = H; b->reduced_depth = red; b->expanded_depth = ex; b->stride = stride;
        b->depth_reduction = carve(&c, inc * red, 2.0 / (double)(inc + red));
        b->norm_depth_reduction = make_bn(&c, H, red);
        b->spatial = carve(&c, red * red * 9, 2.0 / (9.0 * (red + red)));
        b->norm_spatial = make_bn(&c, H / stride, red);
        b->depth_expansion = carve(&c, ex * red, 2.0 / (double)(red + ex));
        b->norm_expansion = make_bn(&c, H / stride, ex);
        if (inc != ex) { /* resnet.cu:770-793: 3x3 stride-2 projection when the block strides, else 1x1 */
            if (stride == 2) b->projection = carve(&c, 9 * inc * ex, 2.0 / (9.0 * (inc + ex)));
            else b->projection = carve(&c, inc * ex, 2.0 / (double)(inc + ex));
            b->norm_projection = make_bn(&c, H / stride, ex);
        }
        p->conv_blocks[i] = b;
        if (stride == 2) H /= 2;
        inc = ex;
    }
    p->fully_connected = carve(&c, ex * d->output, 1e-4); /* resnet.cu:938 */
    p->locations = c.loc; p->sizes = c.sizes; p->n_locations = c.n;

    MiGlobal *g = mi_global();
    mid_memset(c.base, 0, arena_floats * sizeof(float), g->compute);
    if (gen) {
        /* tensor i draws from the stream at offset sum(sizes[0..i)) -- same rule as tests/synth.make_params */
        size_t off = 0, maxsz = 0;
        for (int i = 0; i < c.n; i++) if ((size_t)c.sizes[i] > maxsz) maxsz = c.sizes[i];
        float *host = (float *)malloc(maxsz * sizeof(float));
        for (int i = 0; i < c.n; i++) {
            const size_t sz = c.sizes[i];
            if (c.var[i] > 0) mi_synth_normal(host, sz, gen->seed, gen->counter + off, c.var[i]);
            else if (c.var[i] < 0) for (size_t j = 0; j < sz; j++) host[j] = 1.0f;
            if (c.var[i] != 0) { mid_memcpy_h2d(c.loc[i], host, sz * sizeof(float), g->compute); mid_stream_sync(g->compute); }
            off += sz;
        }
        gen->counter += off;
        free(host);
    }
    mid_stream_sync(g->compute);
    free(c.var);
    return p;
}
static void free_params_host(Params *p, const Dims *d) {
    if (!p) return;
    free(p->norm_init_conv);
    for (int i = 0; i < d->n_conv_blocks; i++) {
        ConvBlock *b = p->conv_blocks[i];
        free(b->norm_depth_reduction); free(b->norm_spatial); free(b->norm_expansion); free(b->norm_projection); free(b);
    }
    free(p->conv_blocks); free(p->locations); free(p->sizes); free(p);
}

/* resnet.cu:951-957 */
ResNet *init_resnet(Dims *dims, MiRng *gen) {
    ResNet *m = (ResNet *)malloc(sizeof(ResNet));
    MiRng tmp = {1234, 0};
    m->dims = dims;
    m->params = build_params(dims, gen ? gen : &tmp, NULL);
    return m;
}

/* ---------------------------------------------------------------------------------------------- */
static Cache_BatchNorm *make_cache(MiCtx *c, int input_size, int feature_size, int with_stats) {
    Cache_BatchNorm *k = (Cache_BatchNorm *)calloc(1, sizeof(Cache_BatchNorm));
    k->input_size = input_size; k->feature_size = feature_size;
    if (with_stats) {
        k->means = (float *)mi_ctx_alloc(c, sizeof(float) * feature_size);
        k->vars = (float *)mi_ctx_alloc(c, sizeof(float) * feature_size);
    }
    return k;
}
static float *falloc(MiCtx *c, size_t n) { return (float *)mi_ctx_alloc(c, n * sizeof(float)); }
/* an activation tensor of n elements in the trainer's storage type (the struct fields stay `float *`, resnet.h).  bf16
 * tensors get MI_GUARD bytes of slack on both sides: the bf16 convolution reads a tap-shifted operand with 16-byte loads,
 * which reach up to (W + 1) elements before the first / past the last pixel of a tensor (those lanes are masked to zero) */
static float *aalloc(MiCtx *c, size_t n) {
    if (c->dtype != MID_BF16) return (float *)mi_ctx_alloc(c, n * 4);
    return (float *)((char *)mi_ctx_alloc(c, n * 2 + 2 * MI_GUARD) + MI_GUARD);
}

/* init_activations, resnet.cu:1057-1113.
 * mode 0: the forward tree.  What it keeps follows c->policy (FAST: raw + BN(+ReLU) output per convolution;
 *         RECOMPUTE_BN: the BN(+ReLU) tensors are two shared scratch buffers, re-derived in backward).
 * mode 1: the derivative tree over six rolling buffers (resnet_cudnn_lowmem.cu:2152-2170).
 * mode 2: the derivative tree with a buffer of its own per tensor, the reference's full mirror (resnet.cu:1151):
 *         FULL policy, so that a dump of activation_derivs/ holds what its file names say. */
static Activations *build_activations(MiCtx *c, const Dims *d, ConvBlock **blocks, int N, float **pool, int mode) {
    Activations *a = (Activations *)calloc(1, sizeof(Activations));
    const int f = d->init_conv_filters, Hs = d->input / d->init_conv_stride, Hp = Hs / d->init_maxpool_stride;
    const size_t stem = (size_t)N * f * Hs * Hs, pl = (size_t)N * f * Hp * Hp;
    const int rc = mode == 0 && c->policy == MI_STORE_RECOMPUTE_BN;
    a->n_conv_blocks = d->n_conv_blocks;
    a->activation_conv_blocks = (Activation_ConvBlock **)calloc(d->n_conv_blocks > 0 ? d->n_conv_blocks : 1, sizeof(void *));
    if (mode == 0) {
        a->init_conv_applied = falloc(c, stem); /* the 7x7 stem keeps fp32 tensors in every storage type */
        a->norm_init_conv = make_cache(c, (int)stem, f, 1);
        a->init_conv_activated = rc ? c->rc_buf[0] : aalloc(c, stem);
        a->max_inds = (int *)mi_ctx_alloc(c, pl * sizeof(int));
        a->init_convblock_input = aalloc(c, pl);
    } else if (mode == 2) {
        a->init_conv_applied = falloc(c, stem);
        a->norm_init_conv = make_cache(c, (int)stem, f, 0);
        a->init_conv_activated = aalloc(c, stem);
        a->init_convblock_input = aalloc(c, pl);
    } else {
        a->init_conv_applied = c->dtype == MID_BF16 ? c->stem_dx : pool[3]; /* B */
        a->norm_init_conv = make_cache(c, (int)stem, f, 0);
        a->init_conv_activated = pool[2]; /* A */
        a->init_convblock_input = pool[0]; /* U0 */
    }
    for (int i = 0; i < d->n_conv_blocks; i++) {
        const ConvBlock *b = blocks[i];
        Activation_ConvBlock *k = (Activation_ConvBlock *)calloc(1, sizeof(Activation_ConvBlock));
        k->incoming_filters = b->incoming_filters; k->incoming_spatial_dim = b->incoming_spatial_dim;
        k->reduced_depth = b->reduced_depth; k->expanded_depth = b->expanded_depth; k->stride = b->stride;
        const int H = b->incoming_spatial_dim, Ho = H / b->stride;
        const size_t rsz = (size_t)N * b->reduced_depth * H * H, ssz = (size_t)N * b->reduced_depth * Ho * Ho,
                     osz = (size_t)N * b->expanded_depth * Ho * Ho;
        const int has_proj = b->projection != NULL;
        k->norm_post_reduced = make_cache(c, (int)rsz, b->reduced_depth, mode == 0);
        k->norm_post_spatial = make_cache(c, (int)ssz, b->reduced_depth, mode == 0);
        k->norm_post_expanded = make_cache(c, (int)osz, b->expanded_depth, mode == 0);
        if (has_proj) k->norm_post_projection = make_cache(c, (int)osz, b->expanded_depth, mode == 0);
        if (mode == 0) {
            k->post_reduced = aalloc(c, rsz); k->post_reduced_activated = rc ? c->rc_buf[0] : aalloc(c, rsz);
            k->post_spatial = aalloc(c, ssz); k->post_spatial_activated = rc ? c->rc_buf[1] : aalloc(c, ssz);
            k->post_expanded = aalloc(c, osz);
            if (has_proj) { k->transformed_residual = aalloc(c, osz); k->post_projection_norm_vals = rc ? c->rc_buf[0] : aalloc(c, osz); }
            k->output_activated = aalloc(c, osz);
            k->output = k->output_activated; /* pre-ReLU sum is not kept unless full-store */
        } else if (mode == 2) {
            k->output_activated = aalloc(c, osz); k->output = aalloc(c, osz);
            k->transformed_residual = has_proj ? aalloc(c, osz) : NULL;
            k->post_expanded = aalloc(c, osz);
            k->post_spatial_activated = aalloc(c, ssz); k->post_spatial = aalloc(c, ssz);
            k->post_reduced_activated = aalloc(c, rsz); k->post_reduced = aalloc(c, rsz);
        } else {
            /* lifetimes inside one block's backward (see backwards_pass): A,B,C,D scratch + alternating U */
            k->output_activated = pool[(i + 1) & 1];
            k->output = pool[5];               /* D: ReLU'-gated upstream, identity blocks only */
            k->transformed_residual = has_proj ? pool[2] : NULL; /* A */
            k->post_expanded = pool[3];         /* B */
            k->post_spatial_activated = pool[4]; /* C */
            k->post_spatial = pool[2];          /* A */
            k->post_reduced_activated = pool[3]; /* B */
            k->post_reduced = pool[4];          /* C */
        }
        a->activation_conv_blocks[i] = k;
    }
    if (mode == 0) {
        a->final_conv_output_pooled = falloc(c, (size_t)N * d->final_depth);
        a->linear_output = falloc(c, (size_t)N * d->output);
    } else a->final_conv_output_pooled = falloc(c, (size_t)N * d->final_depth);
    return a;
}

static size_t max_tensor_elems(const Dims *d, ConvBlock **blocks, int N) {
    const int f = d->init_conv_filters, Hs = d->input / d->init_conv_stride;
    size_t m = (size_t)N * f * Hs * Hs;
    for (int i = 0; i < d->n_conv_blocks; i++) {
        const ConvBlock *b = blocks[i];
        const int H = b->incoming_spatial_dim, Ho = H / b->stride;
        size_t v[3] = {(size_t)N * b->reduced_depth * H * H, (size_t)N * b->expanded_depth * Ho * Ho,
                       (size_t)N * b->incoming_filters * H * H};
        for (int j = 0; j < 3; j++) if (v[j] > m) m = v[j];
    }
    return m;
}

static MiCtx *ctx_of(Train_ResNet *t) { return (MiCtx *)t->backend_ctx; }
/* The unit table (MiCtx.units, mi_host.h): the one place that says what the network is -- every conv + BN unit's shape, parameters,
 * gradients, and which forward tensors it reads and writes.  build_buffers calls it once the forward tree exists (FULL: with its
 * extras); every pass below reads the table and none walks the trees for these facts again. */
static MiUnit *unit_of(const MiCtx *c, int block, int role) {
    if (role == MI_U_STEM) return c->units;
    MiUnit *u = c->units + c->blk_unit[block] + (role - MI_U_RED);
    return u < c->units + c->n_units && u->block == block ? u : NULL; /* (NULL: no projection) */
}
static MiUnit *unit_new(MiCtx *c, int block, int role, int site, const float *w, int C, int H, int K, int k, int stride, const BatchNorm *bn,
                        BatchNorm *dbn, float *dw, Cache_BatchNorm *cache) {
    MiUnit *u = &c->units[c->n_units++];
    mi_layer_init(&u->L, w, C, H, K, k, stride);
    u->block = block; u->role = role; u->site = site;
    u->bn = bn; u->dbn = dbn; u->dw = dw; u->cache = cache;
    u->rs_off = u == c->units ? 0 : u[-1].rs_off + u[-1].bn->depth;
    return u;
}
static void unit_tensors(MiUnit *u, const float *in, float *conv_out, float *act_out, const float *residual, int relu) {
    u->in = in; u->conv_out = conv_out; u->act_out = u->out = act_out; u->residual = residual; u->relu = relu;
}
static void build_units(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    const Dims *d = t->model->dims;
    const Params *p = t->model->params, *dp = t->backprop_buffer->param_derivs;
    const Activations *a = t->forward_buffer->activations;
    const int nb = d->n_conv_blocks;
    c->units = (MiUnit *)calloc((size_t)(4 * nb + 1), sizeof(MiUnit));
    c->blk_unit = (int *)calloc((size_t)(nb > 0 ? nb : 1), sizeof(int));
    c->n_units = 0;
    MiUnit *stem = unit_new(c, -1, MI_U_STEM, 0, p->init_conv_layer, 3, d->input, d->init_conv_filters, d->init_kernel_dim, d->init_conv_stride,
                            p->norm_init_conv, dp->norm_init_conv, dp->init_conv_layer, a->norm_init_conv);
    unit_tensors(stem, NULL, a->init_conv_applied, a->init_conv_activated, NULL, 1);
    const float *bin = a->init_convblock_input; /* the block's input: the max-pool's output, then the output of the block above */
    MiUnit *above = NULL;                       /* and the expansion unit that wrote it */
    for (int i = 0; i < nb; i++) {
        const ConvBlock *b = p->conv_blocks[i], *db = dp->conv_blocks[i];
        const Activation_ConvBlock *k = a->activation_conv_blocks[i];
        const int H = b->incoming_spatial_dim, s = b->stride, inc = b->incoming_filters, rd = b->reduced_depth, ex = b->expanded_depth;
        c->blk_unit[i] = c->n_units;
        /* BN' sites (mi_layer_plan): the reduction's dgrad feeds the expansion BN' of an identity block below it */
        MiUnit *red = unit_new(c, i, MI_U_RED, i > 0 && !p->conv_blocks[i - 1]->projection ? 4 : 0, b->depth_reduction, inc, H, rd, 1, 1,
                               b->norm_depth_reduction, db->norm_depth_reduction, db->depth_reduction, k->norm_post_reduced);
        MiUnit *spa = unit_new(c, i, MI_U_SPA, 2, b->spatial, rd, H, rd, 3, s, b->norm_spatial, db->norm_spatial, db->spatial, k->norm_post_spatial);
        MiUnit *expa = unit_new(c, i, MI_U_EXP, 1, b->depth_expansion, rd, H / s, ex, 1, 1, b->norm_expansion, db->norm_expansion,
                               db->depth_expansion, k->norm_post_expanded);
        unit_tensors(red, bin, k->post_reduced, k->post_reduced_activated, NULL, 1);
        unit_tensors(spa, red->out, k->post_spatial, k->post_spatial_activated, NULL, 1);
        red->cl_reader = spa; /* the reduction BN writes the 3x3's planes beside its NCHW output */
        const float *res = bin;
        if (b->projection) { /* resnet.cu:1685-1704; 3x3 where the block strides */
            MiUnit *proj = unit_new(c, i, MI_U_PROJ, 0, b->projection, inc, H, ex, s == 2 ? 3 : 1, s, b->norm_projection, db->norm_projection,
                                    db->projection, k->norm_post_projection);
            unit_tensors(proj, bin, k->transformed_residual, k->post_projection_norm_vals, NULL, 0);
            /* this block's input is the output of the block above: its BN + add + ReLU writes the projection's planes too */
            if (above && !above->add) above->cl_reader = proj;
            res = proj->out;
        }
        if (!c->full_store) /* BN(expanded) + addVec + doActivation in one kernel (:1670, :1717, :1723) */
            unit_tensors(expa, spa->out, k->post_expanded, k->output_activated, res, 0);
        else { /* the BN output and the pre-ReLU sum are kept: the add is a pass of its own */
            unit_tensors(expa, spa->out, k->post_expanded, k->post_expanded_norm_vals, NULL, 0);
            expa->add = res; expa->sum = k->output; expa->out = k->output_activated;
        }
        bin = expa->out; above = expa;
    }
}
/* every unit's convolution planned and given its buffers by layer.c; what the network adds is who writes a layer's channel-last planes
 * (cl_by_bn), the table of weights re-laid once per forward pass, and the workspaces sized for the largest layer */
static void plan_layers(MiCtx *c, const Dims *d, int N) {
    MiUnit *const end = c->units + c->n_units;
    MiLayerNeed need = {0, 0, 0, d->init_conv_filters};
    free(c->wt_tab);
    c->wt_tab = (mid_wt_entry *)calloc((size_t)c->n_units, sizeof(mid_wt_entry));
    c->wt_n = 0; c->wt_tiles = 0;
    for (MiUnit *u = c->units; u < end; u++) {
        MiLayer *L = &u->L;
        ck(mi_layer_plan(L, c->dtype, c->policy, &c->opt, N, u->site, NULL), "convolution plan");
        mi_layer_alloc(c, L);
        mi_layer_need(L, &need);
        if (!L->wre_fwd && !L->wre_dgrad) continue;
        mid_wt_entry *e = &c->wt_tab[c->wt_n++];
        e->w = L->w; e->K = L->K; e->C = L->C; e->T = L->k * L->k;
        e->fwd = L->wre_fwd ? falloc(c, L->wre_floats) : NULL; e->dgrad = L->wre_dgrad ? falloc(c, L->wre_floats) : NULL;
        e->tile0 = c->wt_tiles; c->wt_tiles += (L->C / 32) * (L->K / 32);
        L->we = e;
    }
    c->stem_bf16 = c->units->L.out_dt == MID_BF16;
    for (MiUnit *u = c->units; u < end; u++) { /* (stride 2: a re-layout pass instead where the plane is odd) */
        MiLayer *R = u->cl_reader ? &u->cl_reader->L : NULL;
        if (R && R->cl) R->cl_by_bn = R->stride == 1 || !(R->H & 1);
    }
    c->wt_tab_dev = NULL; c->wt_tile_entry_dev = NULL;
    if (c->wt_n) {
        int *te = (int *)malloc((size_t)c->wt_tiles * sizeof(int));
        for (int e = 0; e < c->wt_n; e++) {
            const int nt = (c->wt_tab[e].C / 32) * (c->wt_tab[e].K / 32);
            for (int q = 0; q < nt; q++) te[c->wt_tab[e].tile0 + q] = e;
        }
        c->wt_tab_dev = (mid_wt_entry *)mi_ctx_alloc(c, (size_t)c->wt_n * sizeof(mid_wt_entry));
        c->wt_tile_entry_dev = (int *)mi_ctx_alloc(c, (size_t)c->wt_tiles * sizeof(int));
        mid_memcpy_h2d(c->wt_tab_dev, c->wt_tab, (size_t)c->wt_n * sizeof(mid_wt_entry), G.compute);
        mid_memcpy_h2d(c->wt_tile_entry_dev, te, (size_t)c->wt_tiles * sizeof(int), G.compute);
        mid_stream_sync(G.compute);
        free(te);
    }
    mi_layer_ws_alloc(c, &c->lw, &need);
}

static void free_activations_host(Activations *a);
static void add_full_store_extras(Train_ResNet *t);
static void rs_build_table(Train_ResNet *t);
/* everything whose size or layout depends on the storage type / store policy: activation trees, derivative buffers,
 * workspaces, re-laid weight tables.  Called by init_trainer and again by mi_trainer_set_dtype / _set_store_policy. */
static void build_buffers(Train_ResNet *t) {
    MiCtx *c = (MiCtx *)t->backend_ctx;
    Dims *d = t->model->dims;
    ConvBlock **blocks = t->model->params->conv_blocks;
    const int N = t->batch_size;
    const size_t maxe = max_tensor_elems(d, blocks, N);
    c->act_bytes = 0;
    c->rc_buf[0] = c->rc_buf[1] = NULL;
    if (c->policy == MI_STORE_RECOMPUTE_BN) { c->rc_buf[0] = aalloc(c, maxe); c->rc_buf[1] = aalloc(c, maxe); }
    c->counting_act = 1;
    t->forward_buffer->activations = build_activations(c, d, blocks, N, NULL, 0);
    c->counting_act = 0;
    c->full_store = 0;
    if (c->policy == MI_STORE_FULL) add_full_store_extras(t);
    const int f = d->init_conv_filters, Hs = d->input / d->init_conv_stride;
    c->stem_dx = c->dtype == MID_BF16 ? falloc(c, (size_t)N * f * Hs * Hs) : NULL;
    float *pool[6];
    for (int i = 0; i < 6; i++) pool[i] = aalloc(c, maxe);
    for (int i = 0; i < 6; i++) c->dpool[i] = pool[i];
    for (int i = 0; i < MI_RING; i++) { c->ring_buf[i] = i < 4 ? pool[2 + i] : aalloc(c, maxe); c->ring_busy[i] = 0; }
    c->ring_next = 0;
    t->backprop_buffer->activation_derivs = build_activations(c, d, blocks, N, pool, c->policy == MI_STORE_FULL ? 2 : 1);
    /* ring mode re-points derivative tensors to equal-sized slots: FAST policy and fp32 only (the bf16 path keeps the stem's
     * fp32 gradient in a buffer of its own) */
    if ((c->policy != MI_STORE_FAST || c->dtype != MID_F32) && c->overlap_wgrad > 1) c->overlap_wgrad = 1;
    /* bf16: the weight gradients are no longer bound by the matrix pipe but by memory, like the batch norm they would run
     * next to -- measured 6028 img/s serial against 5973 overlapped; an explicit RESNET_MI_OVERLAP still wins */
    if (c->dtype == MID_BF16 && !c->opt.overlap_given && !c->overlap_set) c->overlap_wgrad = 0;
    build_units(t);
    plan_layers(c, d, N);
    mid_stream_sync(G.compute);
    rs_build_table(t); /* (the caches the running-statistics table points at were rebuilt) */
}
static void drop_buffers(Train_ResNet *t) {
    MiCtx *c = (MiCtx *)t->backend_ctx;
    mid_device_sync();
    ctx_free_from(c, c->n_persist);
    free_activations_host(t->forward_buffer->activations);
    free_activations_host(t->backprop_buffer->activation_derivs);
    t->forward_buffer->activations = NULL; t->backprop_buffer->activation_derivs = NULL;
    c->wt_n = 0; c->wt_tiles = 0; c->wt_tab_dev = NULL; c->wt_tile_entry_dev = NULL;
    c->wgrad_pending = 0;
    free(c->units); free(c->blk_unit); /* the table pointed into what was just freed */
    c->units = NULL; c->blk_unit = NULL; c->n_units = 0;
}

/* the trainer's switches (MiOptions), read once per trainer: a trainer made after a change of the environment sees the change */
void mi_read_options(MiOptions *o) {
#define ENV_INT(name_, default_) (getenv(name_) ? atoi(getenv(name_)) : (default_))
    o->cl_s1 = ENV_INT("RESNET_MI_BF16_CL_S1", 1) != 0;
    o->cl_s1_dgrad = ENV_INT("RESNET_MI_BF16_CL_S1_DGRAD", 1) != 0;
    o->cl_s2 = ENV_INT("RESNET_MI_BF16_CL_S2", 1) != 0;
    o->cl_dgrad2 = ENV_INT("RESNET_MI_BF16_CL_DGRAD2", 1) != 0;
    o->stem_mfma = ENV_INT("RESNET_MI_STEM_MFMA", 1) != 0;
    o->bf16_stem = ENV_INT("RESNET_MI_BF16_STEM", 1) != 0;
    o->stem_tensors_f32 = getenv("RESNET_MI_BF16_STEM_TENSORS") && !strcmp(getenv("RESNET_MI_BF16_STEM_TENSORS"), "f32");
    o->bnfuse_bwd = ENV_INT("RESNET_MI_BF16_BNFUSE_BWD", 1) != 0;
    o->bnfuse_bwd_f32 = ENV_INT("RESNET_MI_F32_BNFUSE_BWD", 4);
    o->overlap = ENV_INT("RESNET_MI_OVERLAP", 1);
    o->overlap_given = getenv("RESNET_MI_OVERLAP") != NULL;
    o->bnfuse = ENV_INT("RESNET_MI_BNFUSE", 1);
    o->prelayout = ENV_INT("RESNET_MI_PRELAYOUT", 1);
    o->igemm = ENV_INT("RESNET_MI_IGEMM", 2);
    o->pw_wgrad = ENV_INT("RESNET_MI_BF16_PW_WGRAD", 1) != 0;
#undef ENV_INT
}
/* resnet.cu:1157-1194 */
Train_ResNet *init_trainer(ResNet *model, Batch *cur_batch, int batch_size, float learning_rate, float weight_decay,
                           float mean_decay, float var_decay, float eps, int n_epochs, const char *dump_dir) {
    Train_ResNet *t = (Train_ResNet *)calloc(1, sizeof(Train_ResNet));
    MiCtx *c = (MiCtx *)calloc(1, sizeof(MiCtx));
    Dims *d = model->dims;
    mi_global();
    t->backend_ctx = c;
    t->model = model; t->cur_batch = cur_batch; t->batch_size = batch_size;
    c->dump_every = 1000; /* resnet.cu:2947 */
    c->input_reset = 1;   /* resnet.cu:2981-2982 */
    c->world = 1; c->bucket_bytes = (size_t)32 << 20;
    c->dtype = MID_F32; c->policy = MI_STORE_FAST;
    mi_read_options(&c->opt);
    c->overlap_wgrad = c->opt.overlap;
    c->ev_bn_done = mid_event_create(); c->ev_wgrad_done = mid_event_create();

    /* persistent device state: survives a change of storage type / store policy */
    Forward_Buffer *fb = (Forward_Buffer *)calloc(1, sizeof(Forward_Buffer));
    fb->pred = falloc(c, (size_t)batch_size * d->output); /* reference over-allocates N^2*output (:1126, hazard h4) */
    fb->pred_cpu = (float *)mid_malloc_host((size_t)batch_size * d->output * sizeof(float));
    t->forward_buffer = fb;
    Backprop_Buffer *bb = (Backprop_Buffer *)calloc(1, sizeof(Backprop_Buffer));
    bb->output_layer_deriv = falloc(c, (size_t)batch_size * d->output);
    bb->param_derivs = build_params(d, NULL, c);
    bb->prev_means = build_params(d, NULL, c);
    bb->prev_vars = build_params(d, NULL, c);
    t->backprop_buffer = bb;
    c->arena_floats = mi_params_arena_floats(model->params);
    c->g_arena = mi_params_arena_base(bb->param_derivs);
    c->m_arena = mi_params_arena_base(bb->prev_means);
    c->v_arena = mi_params_arena_base(bb->prev_vars);
    { /* arena offsets of the tensors, for the Adam kernel's "which location" report */
        const Params *mp = model->params;
        size_t *lo = (size_t *)malloc(sizeof(size_t) * (size_t)(mp->n_locations + 1));
        for (int i = 0; i < mp->n_locations; i++) lo[i] = (size_t)(mp->locations[i] - mp->locations[0]);
        lo[mp->n_locations] = c->arena_floats;
        c->loc_off_dev = (size_t *)mi_ctx_alloc(c, sizeof(size_t) * (size_t)(mp->n_locations + 1));
        mid_memcpy_h2d(c->loc_off_dev, lo, sizeof(size_t) * (size_t)(mp->n_locations + 1), G.compute);
        mid_stream_sync(G.compute);
        c->loc_off = lo;
        c->n_loc = mp->n_locations;
    }
    c->ev_nan = mid_event_create();
    c->nan_location = -1;
    c->acc_k = 1; c->acc_scale = 1.f; /* no accumulation: every update_parameters applies its own gradient */
    c->loss_topk = 1; /* with smoothing 0 and MI_LOSS_HOST: the reference's head */
    c->loss_row = falloc(c, (size_t)batch_size);
    c->loss_rank = (int *)mi_ctx_alloc(c, (size_t)batch_size * sizeof(int));
    c->loss_metrics = (mid_loss_metrics *)mi_ctx_alloc(c, 2 * sizeof(mid_loss_metrics));
    mid_memset(c->loss_metrics, 0, 2 * sizeof(mid_loss_metrics), G.compute);
    c->next_live = g_live; g_live = c;
    c->nan_flag_dev = (int *)mi_ctx_alloc(c, sizeof(int));
    c->nan_flag_host = (int *)mid_malloc_host(sizeof(int));
    *c->nan_flag_host = 0;
    mid_memset(c->nan_flag_dev, 0, sizeof(int), G.compute);
    c->n_persist = c->n_allocs;
    for (int i = 0; i < MI_RING; i++) c->ring_ev[i] = mid_event_create();
    c->ev_grads = mid_event_create(); c->ev_reduced = mid_event_create();
    for (int i = 0; i < 6; i++) c->ev_t[i] = mid_event_create();
    for (int i = 0; i < MI_MAX_BUCKETS; i++) c->bk_ev[i] = mid_event_create();

    build_buffers(t);

    t->learning_rate = learning_rate; t->weight_decay = weight_decay;
    t->base_mean_decay = mean_decay; t->base_var_decay = var_decay;
    t->cur_mean_decay = 1; t->cur_var_decay = 1;
    t->eps = eps; t->n_epochs = n_epochs; t->cur_dump_id = -1; t->cur_epoch = 0;
    t->loss_per_epoch = (float *)calloc(n_epochs > 0 ? n_epochs : 1, sizeof(float));
    t->accuracy_per_epoch = (float *)calloc(n_epochs > 0 ? n_epochs : 1, sizeof(float));
    t->init_loaded = 0;
    t->dump_dir = dump_dir;
    mid_stream_sync(G.compute);
    return t;
}
Train_ResNet *init_trainer_cudnn_abi(ResNet *model, Batch *cur_batch, int batch_size, float learning_rate,
                                     float weight_decay, float mean_decay, float var_decay, float eps, int n_epochs,
                                     void *handle, const char *dump_dir) {
    (void)handle;
    return init_trainer(model, cur_batch, batch_size, learning_rate, weight_decay, mean_decay, var_decay, eps, n_epochs, dump_dir);
}

/* FULL policy: x-hat, BN output and pre-ReLU sums as the reference stores them (dump parity; fp32 only) */
static void add_full_store_extras(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    Activations *a = t->forward_buffer->activations;
    c->counting_act = 1;
#define EXTRA(cache) do { (cache)->normalized_temp = falloc(c, (cache)->input_size); (cache)->normalized = falloc(c, (cache)->input_size); } while (0)
    EXTRA(a->norm_init_conv);
    for (int i = 0; i < a->n_conv_blocks; i++) {
        Activation_ConvBlock *k = a->activation_conv_blocks[i];
        EXTRA(k->norm_post_reduced); EXTRA(k->norm_post_spatial); EXTRA(k->norm_post_expanded);
        if (k->norm_post_projection) EXTRA(k->norm_post_projection);
        k->post_expanded_norm_vals = falloc(c, k->norm_post_expanded->input_size);
        k->output = falloc(c, k->norm_post_expanded->input_size);
    }
#undef EXTRA
    c->counting_act = 0;
    c->full_store = 1;
}
/* every convolution of the bottleneck blocks must tile for the bf16 NCHW kernels (the stem stays on the fp32 path): the planner's own
 * test of those routes, over the table of the trainer's current storage type (the shapes are the same) */
static int bf16_net_supported(const Train_ResNet *t, char *why, size_t whylen) {
    const MiCtx *c = (const MiCtx *)t->backend_ctx;
    const int nchw[3] = {MI_FWD_BF16, MI_DG_BF16, MI_WG_BF16};
    for (const MiUnit *u = c->units + 1; u < c->units + c->n_units; u++) {
        MiLayer L = u->L;
        if (mi_layer_plan(&L, MID_BF16, c->policy, &c->opt, t->batch_size, 0, nchw)) {
            snprintf(why, whylen, "block %d conv %d (C=%d H=%d K=%d k=%d s=%d) does not tile for the bf16 kernels", u->block, u->role - MI_U_RED, L.C, L.H, L.K, L.k, L.stride);
            return 0;
        }
    }
    return 1;
}
void mi_record_host_error(const char *what, const char *detail);
int mi_trainer_set_store_policy(Train_ResNet *t, int policy) {
    MiCtx *c = ctx_of(t);
    if (policy < MI_STORE_FAST || policy > MI_STORE_FULL) { mi_record_host_error("mi_trainer_set_store_policy", "unknown policy"); return -1; }
    if (policy == MI_STORE_FULL && c->dtype != MID_F32) { mi_record_host_error("mi_trainer_set_store_policy", "the FULL policy (x-hat / BN-out / pre-ReLU sums) exists in fp32 only"); return -1; }
    if (policy == c->policy) return 0;
    drop_buffers(t);
    c->policy = policy;
    build_buffers(t);
    return 0;
}
void mi_trainer_set_full_store(Train_ResNet *t, int on) { (void)mi_trainer_set_store_policy(t, on ? MI_STORE_FULL : MI_STORE_FAST); }
int mi_trainer_set_dtype(Train_ResNet *t, int dtype) {
    MiCtx *c = ctx_of(t);
    if (dtype != MID_F32 && dtype != MID_BF16) { mi_record_host_error("mi_trainer_set_dtype", "unknown dtype"); return -1; }
    if (dtype == c->dtype) return 0;
    if (dtype == MID_BF16) {
        char why[256];
        if (c->policy == MI_STORE_FULL) { mi_record_host_error("mi_trainer_set_dtype", "the FULL store policy exists in fp32 only"); return -1; }
        if (!bf16_net_supported(t, why, sizeof why)) { mi_record_host_error("mi_trainer_set_dtype", why); return -1; }
    }
    drop_buffers(t);
    c->dtype = dtype;
    build_buffers(t);
    return 0;
}
int mi_trainer_get_dtype(const Train_ResNet *t) { return ((MiCtx *)t->backend_ctx)->dtype; }
size_t mi_trainer_activation_bytes(const Train_ResNet *t) { return ((MiCtx *)t->backend_ctx)->act_bytes; }
size_t mi_trainer_device_bytes(const Train_ResNet *t) {
    const MiCtx *c = (MiCtx *)t->backend_ctx;
    const size_t ema = c->ema_arena ? (c->arena_floats + 2 * (size_t)c->rs_channels) * sizeof(float) : 0; /* mi_trainer_set_ema's two arenas */
    const size_t acc = c->acc_arena ? c->arena_floats * sizeof(float) : 0; /* mi_trainer_set_accumulation's arena */
    return c->dev_bytes + c->arena_floats * sizeof(float) + ema + acc + c->clip.bytes; /* + the parameter arena (owned by the model); + mi_trainer_set_clip_grad_norm's table */
}
void mi_trainer_set_dump_every(Train_ResNet *t, int every) { ctx_of(t)->dump_every = every; }
void mi_trainer_set_overlap(Train_ResNet *t, int mode) {
    MiCtx *c = ctx_of(t);
    mid_stream_sync(G.aux); mid_stream_sync(G.compute);
    c->overlap_wgrad = mode < 0 ? 0 : mode > 2 ? 2 : mode;
    c->overlap_set = 1;
    if ((c->policy != MI_STORE_FAST || c->dtype != MID_F32) && c->overlap_wgrad > 1) c->overlap_wgrad = 1; /* the ring re-points derivative tensors */
    c->wgrad_pending = 0;
    for (int i = 0; i < MI_RING; i++) c->ring_busy[i] = 0;
    if (c->overlap_wgrad != 2) { /* back to the fixed aliasing of build_activations */
        Activations *da = t->backprop_buffer->activation_derivs;
        float **pool = c->dpool;
        if (c->policy == MI_STORE_FULL) return; /* every derivative tensor has a buffer of its own */
        da->init_conv_applied = c->dtype == MID_BF16 ? c->stem_dx : pool[3]; da->init_conv_activated = pool[2];
        for (int i = 0; i < da->n_conv_blocks; i++) {
            Activation_ConvBlock *k = da->activation_conv_blocks[i];
            k->output = pool[5];
            if (k->transformed_residual) k->transformed_residual = pool[2];
            k->post_expanded = pool[3]; k->post_spatial_activated = pool[4]; k->post_spatial = pool[2];
            k->post_reduced_activated = pool[3]; k->post_reduced = pool[4];
        }
    }
}
void mi_trainer_set_input_reset(Train_ResNet *t, int on) { ctx_of(t)->input_reset = on; }
void mi_trainer_set_dump_root(Train_ResNet *t, const char *root) {
    MiCtx *c = ctx_of(t);
    free(c->dump_root);
    c->dump_root = root ? strdup(root) : NULL;
}
void mi_trainer_last_timings(Train_ResNet *t, float out_ms[5]) {
    MiCtx *c = ctx_of(t);
    mid_stream_sync(G.compute);
    out_ms[0] = 0;
    out_ms[1] = mid_event_elapsed_ms(c->ev_t[0], c->ev_t[1]);
    out_ms[2] = mid_event_elapsed_ms(c->ev_t[2], c->ev_t[3]);
    out_ms[3] = mid_event_elapsed_ms(c->ev_t[4], c->ev_t[5]);
    out_ms[4] = c->last_ms[4];
}

/* ---------------------------------------------------------------------------------------------- */
/* every implicit-GEMM layer's weights in the layouts forward and dgrad want, one launch (they hold until the parameters
 * change: update_parameters, or a host write -- mi_copy_to_device / overwrite_model_params set the dirty flag) */
static void relayout_weights(MiCtx *c) {
    if (c->dtype == MID_BF16) ck(mid_conv_prelayout_all_bf16(G.compute, c->wt_tab_dev, c->wt_tile_entry_dev, c->wt_tiles), "weight re-layout (bf16)");
    else ck(mid_conv_prelayout_all(G.compute, c->wt_tab_dev, c->wt_tile_entry_dev, c->wt_tiles), "weight re-layout");
    c->params_dirty = 0;
    c->host_epoch_seen = g_host_write_epoch;
}
static int weights_stale(const MiCtx *c) { return c->params_dirty || c->host_epoch_seen != g_host_write_epoch; }
/* the NaN / Inf flag update_parameters queued a copy of; valid after any later synchronisation of the compute stream
 * (check_errors, resnet.cu:2879-2907: dump id 99999999 and exit; offending gradients are still in the arena, the Adam
 * kernel clears only finite ones) */
void dump_trainer(int dump_id, Train_ResNet *trainer, const char *special_dir);
static void poll_nan_flag(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    if (!c->nan_check_pending) return;
    c->nan_check_pending = 0;
    if (*c->nan_flag_host) {
        /* the Adam kernel left (highest offending locations[] index + 1): the tensor check_errors would have named first,
         * walking locations[] from the last to the first (resnet.cu:2896, :2952) */
        printf("ERROR: nan or inf found at location: %d\n", *c->nan_flag_host - 1);
        printf("Dumping data to id=99999999 and exiting...\n");
        c->nan_location = *c->nan_flag_host - 1;
        if (c->dp_pending) mid_stream_sync(G.comm);
        dump_trainer(99999999, t, t->dump_dir);
        if (c->nan_no_exit) { /* test hook: report through mi_trainer_check_errors instead of exiting; the run goes on from a clean flag */
            mid_memset(c->nan_flag_dev, 0, sizeof(int), G.compute);
            mid_stream_sync(G.compute);
            *c->nan_flag_host = 0;
            return;
        }
        abort_all_comms(); /* do not leave the peers waiting in a collective */
        exit(1);
    }
}
/* load_new_batch calls this before it replaces the batch: the flag copy update_parameters queued is waited for (one event, the
 * step is over by then), so that a 99999999 dump holds the OFFENDING step's inputs, activations and dump id -- what
 * resnet.cu:2879-2907 dumps from inside update_parameters */
void mi_trainer_poll_errors(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    if (!c || !c->nan_check_pending) return;
    mid_event_sync(c->ev_nan);
    poll_nan_flag(t);
}

/* conv + BN (+ReLU | +residual+ReLU): prepareAndDoConvolution + prepareAndDoBatchNormAndActivate.
 * stem: the 7x7 convolution keeps fp32 input / output in every storage type; only its BN output is an activation tensor.
 * running 0: the batch's statistics, left in the unit's cache; 1: the unit's running statistics, read only -- the same convolution call
 * (its statistics partials are left unused), then the apply kernel alone */
static void unit_fwd(Train_ResNet *t, MiUnit *u, const float *images, int running) {
    MiCtx *c = ctx_of(t);
    MiLayer *L = &u->L;
    const BatchNorm *bn = u->bn;
    const MiLayer *reader = u->cl_reader ? &u->cl_reader->L : NULL;
    /* the convolution leaves per-tile (count, mean, M2) partials of its output: BN reads the tensor twice, not three times (the
     * kernels with bf16 operands always do) */
    const int bf_ops = L->fwd == MI_FWD_BF16 || L->fwd == MI_FWD_CL || L->fwd == MI_FWD_STEM_BF16;
    mid_bn_parts *parts = (c->opt.bnfuse || bf_ops) ? &c->lw.bn_parts : NULL;
    ck(mi_layer_fwd(L, &c->lw, G.compute, u->in ? u->in : images, u->conv_out, parts), "convolution forward");
    if (running) {
        const float *rm = c->rs_arena + u->rs_off, *rv = rm + c->rs_channels;
        ck(mi_layer_bn_apply(L, G.compute, u->conv_out, bn->gamma, bn->beta, u->residual, rm, rv, u->act_out, t->eps, u->relu, reader),
           "batch norm (running statistics)");
    } else
        ck(mi_layer_bn_fwd(L, &c->lw, G.compute, parts, u->conv_out, bn->gamma, bn->beta, u->residual, u->cache->means, u->cache->vars, u->act_out,
                           u->cache->normalized_temp, u->cache->normalized, t->eps, u->relu, reader), "batch norm forward");
    if (u->add) { /* FULL policy, expansion */
        const int Ho = L->H / L->stride;
        ck(mid_add_relu(G.compute, u->act_out, u->add, u->sum, u->out, (size_t)L->N * L->K * Ho * Ho), "add + ReLU");
    }
}

/* the batch-norm launchers take their cross-replica setting from one process-wide slot (kernels_bn.hip): every pass binds ITS
 * trainer's (none for a trainer without sync-BN), so two trainers in one process do not inherit each other's */
#define MI_SYNC_BN_TMP_FLOATS (2 * 4096)
static void bind_sync_bn(const MiCtx *c) {
    if (c->sync_bn && c->sync_bn_comm) mid_bn_set_sync(c->sync_bn_comm, c->world, c->sync_bn_tmp, MI_SYNC_BN_TMP_FLOATS, 1);
    else mid_bn_set_sync(NULL, 1, NULL, 0, 0);
}
/* resnet.cu:1526-1775 up to the logits, for forward_pass (running 0) and the eval pass (running 1, see unit_fwd) */
static void forward_trunk(Train_ResNet *t, const float *images, int running) {
    MiCtx *c = ctx_of(t);
    const Dims *d = t->model->dims;
    const Params *p = t->model->params;
    Activations *a = t->forward_buffer->activations;
    const int N = t->batch_size, nb = d->n_conv_blocks;
    relayout_weights(c);
    unit_fwd(t, unit_of(c, -1, MI_U_STEM), images, running);
    ck(mid_maxpool_fwd_t(G.compute, a->init_conv_activated, a->init_convblock_input, c->dtype, a->max_inds, N, d->init_conv_filters,
                         d->input / d->init_conv_stride, d->init_maxpool_dim, d->init_maxpool_stride), "max-pool forward");
    for (int i = 0; i < nb; i++) { /* the table keeps the order of Params.locations; the projection runs before the expansion that adds it */
        unit_fwd(t, unit_of(c, i, MI_U_RED), images, running);
        unit_fwd(t, unit_of(c, i, MI_U_SPA), images, running);
        if (unit_of(c, i, MI_U_PROJ)) unit_fwd(t, unit_of(c, i, MI_U_PROJ), images, running);
        unit_fwd(t, unit_of(c, i, MI_U_EXP), images, running);
    }
    if (!running && c->rs_on) { /* behind the last BN of the pass (under sync-BN: the merged statistics), every unit's running statistics in one launch */
        ck(mid_bn_running_update(G.compute, c->rs_tab_dev, c->n_units, c->rs_channels, c->rs_arena, (size_t)c->rs_channels, c->rs_momentum),
           "running statistics");
        c->rs_updates++;
    }
    const int Hl = p->conv_blocks[nb - 1]->incoming_spatial_dim; /* resnet.cu:1732 */
    ck(mid_avgpool_fwd_t(G.compute, unit_of(c, nb - 1, MI_U_EXP)->out, c->dtype, a->final_conv_output_pooled, N, d->final_depth, Hl * Hl), "average pool");
    ck(mid_gemm_nn(G.compute, a->final_conv_output_pooled, p->fully_connected, a->linear_output, N, d->final_depth, d->output), "FC forward");
}
void forward_pass(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    const Dims *d = t->model->dims;
    Activations *a = t->forward_buffer->activations;
    const int N = t->batch_size;
    mid_event_record(c->ev_t[0], G.compute);
    bind_sync_bn(c);
    c->acts_from_eval = 0;
    c->acc_in_step = 1; /* until update_parameters: mi_trainer_set_accumulation is refused in between */
    forward_trunk(t, t->cur_batch->images, 0);
    if (c->mix_on && c->mix_last.mode != 0) /* the batch was mixed by load_new_batch: both labels of every row, weighted lam / 1 - lam */
        ck(mid_loss_head_mix(G.compute, a->linear_output, t->cur_batch->correct_classes, c->mix_labels_b, c->mix_last.lam, t->forward_buffer->pred,
                             t->backprop_buffer->output_layer_deriv, c->loss_row, c->loss_rank, N, d->output, c->loss_smoothing, c->loss_topk,
                             c->loss_metrics, c->loss_metrics + 1), "two-label loss head");
    else if (c->loss_flags & MI_LOSS_DEVICE) /* soft-max, dlogits (backwards_pass launches no ce_deriv), row losses and ranks, the two records */
        ck(mid_loss_head(G.compute, a->linear_output, t->cur_batch->correct_classes, t->forward_buffer->pred, t->backprop_buffer->output_layer_deriv,
                         c->loss_row, c->loss_rank, N, d->output, c->loss_smoothing, c->loss_topk, c->loss_metrics, c->loss_metrics + 1), "loss head");
    else ck(mid_softmax(G.compute, a->linear_output, t->forward_buffer->pred, N, d->output), "soft-max");
    mid_event_record(c->ev_t[1], G.compute);
    if (c->loss_flags & MI_LOSS_NO_PRED_COPY) { /* nothing the host reads: the queue is not drained, only the flag's own event waited for */
        mi_trainer_poll_errors(t);
        return;
    }
    mid_memcpy_d2h(t->forward_buffer->pred_cpu, t->forward_buffer->pred, (size_t)N * d->output * sizeof(float), G.compute);
    mid_stream_sync(G.compute); /* the reference's blocking cudaMemcpy (:1774) */
    poll_nan_flag(t);           /* the previous update's flag copy has landed by now */
}

/* the head of forward_pass / backwards_pass (resnet_mi.h) */
int mi_trainer_set_loss(Train_ResNet *t, float smoothing, int topk, int flags) {
    MiCtx *c = ctx_of(t);
    if (flags & ~(MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY)) { mi_record_host_error("mi_trainer_set_loss", "unknown flag bits"); return -1; }
    if (mi_loss_args_ok("mi_trainer_set_loss", smoothing, topk, t->model->dims->output)) return -1;
    if (smoothing > 0.f && !(flags & MI_LOSS_DEVICE)) {
        mi_record_host_error("mi_trainer_set_loss", "label smoothing needs MI_LOSS_DEVICE (the host head has none)");
        return -1;
    }
    if ((flags & MI_LOSS_NO_PRED_COPY) && !(flags & MI_LOSS_DEVICE)) {
        mi_record_host_error("mi_trainer_set_loss", "MI_LOSS_NO_PRED_COPY needs MI_LOSS_DEVICE (the host loss reads pred_cpu)");
        return -1;
    }
    if (c->mix_on && !(flags & MI_LOSS_DEVICE)) {
        mi_record_host_error("mi_trainer_set_loss", "mixing is on (mi_trainer_set_mix): the host head has one label per row");
        return -1;
    }
    c->loss_smoothing = smoothing; c->loss_topk = topk; c->loss_flags = flags;
    return 0;
}
/* mixup / CutMix (resnet_mi.h, "mixing") */
int mi_trainer_set_mix(Train_ResNet *t, double mixup_alpha, double cutmix_alpha, double prob, double switch_prob, uint64_t seed) {
    MiCtx *c = ctx_of(t);
    if (mixup_alpha == 0 && cutmix_alpha == 0) { c->mix_on = 0; memset(&c->mix_last, 0, sizeof c->mix_last); return 0; }
    if (!(c->loss_flags & MI_LOSS_DEVICE)) {
        mi_record_host_error("mi_trainer_set_mix", "mixing needs MI_LOSS_DEVICE (mi_trainer_set_loss): the host head has one label per row");
        return -1;
    }
    MiMixPlan probe; /* the argument rules are mi_mix_plan's */
    if (mi_mix_plan(seed, 0, 0, 0, 1, mixup_alpha, cutmix_alpha, prob, switch_prob, t->model->dims->input, &probe)) return -1;
    if (!c->mix_labels_b) c->mix_labels_b = (int *)mid_malloc(sizeof(int) * (size_t)t->batch_size);
    if (!c->mix_labels_b) { mi_record_host_error("mi_trainer_set_mix", "no device memory for the second labels"); return -1; }
    c->mix_alpha[0] = mixup_alpha; c->mix_alpha[1] = cutmix_alpha; c->mix_prob = prob; c->mix_switch = switch_prob; c->mix_seed = seed;
    memset(&c->mix_last, 0, sizeof c->mix_last);
    c->mix_on = 1;
    return 0;
}
int mi_trainer_last_mix(const Train_ResNet *t, MiMixPlan *out) {
    const MiCtx *c = ctx_of((Train_ResNet *)t);
    if (!c->mix_on || !out) { mi_record_host_error("mi_trainer_last_mix", "mixing is off (mi_trainer_set_mix)"); return -1; }
    *out = c->mix_last;
    return 0;
}
void mi_trainer_mix_batch(Train_ResNet *t, Batch *b, int rank, int world) {
    MiCtx *c = ctx_of(t);
    if (!c->mix_on) return;
    if (mi_mix_plan(c->mix_seed, t->cur_epoch, t->cur_dump_id, rank, world, c->mix_alpha[0], c->mix_alpha[1], c->mix_prob, c->mix_switch,
                    b->image_dim, &c->mix_last)) { memset(&c->mix_last, 0, sizeof c->mix_last); return; }
    const MiMixPlan *p = &c->mix_last;
    if (p->mode == 0) return;
    ck(mid_mix_batch(G.compute, b->images, b->n_images, (size_t)b->image_size, b->image_dim, p->mode, p->lam, p->y0, p->x0, p->y1, p->x1), "mix");
    ck(mid_mix_labels(G.compute, b->correct_classes, c->mix_labels_b, b->n_images), "mix labels");
}
/* random erasing (resnet_mi.h, "random erasing") */
int mi_trainer_set_erase(Train_ResNet *t, double prob, double scale_lo, double scale_hi, double ratio_lo, double ratio_hi,
                         const MiEraseFill *fill, uint64_t seed) {
    MiCtx *c = ctx_of(t);
    if (prob == 0) { c->erase_on = 0; c->erase_rows = 0; return 0; }
    if (!fill) { mi_record_host_error("mi_trainer_set_erase", "fill is NULL"); return -1; }
    /* the argument rules are mi_erase_plan's and the kernel's */
    if (mi_erase_plan(seed, 0, 0, 0, 1, 0, t->model->dims->input, prob, scale_lo, scale_hi, ratio_lo, ratio_hi, NULL)) return -1;
    if (!mid_erase_fill_ok("mi_trainer_set_erase", fill->mode, fill->value, fill->std)) return -1;
    if (!c->erase_last) c->erase_last = (int *)calloc((size_t)t->batch_size * 4, sizeof(int));
    if (!c->erase_last) { mi_record_host_error("mi_trainer_set_erase", "no memory for the boxes"); return -1; }
    c->erase_prob = prob; c->erase_scale[0] = scale_lo; c->erase_scale[1] = scale_hi; c->erase_ratio[0] = ratio_lo; c->erase_ratio[1] = ratio_hi;
    c->erase_fill = *fill; c->erase_fill.noise_seed = 0; c->erase_seed = seed;
    c->erase_rows = 0;
    c->erase_on = 1;
    return 0;
}
int mi_trainer_last_erase(const Train_ResNet *t, int *out) {
    const MiCtx *c = ctx_of((Train_ResNet *)t);
    if (!c->erase_on || !out) { mi_record_host_error("mi_trainer_last_erase", "erasing is off (mi_trainer_set_erase)"); return -1; }
    memcpy(out, c->erase_last, (size_t)c->erase_rows * 4 * sizeof(int));
    return c->erase_rows;
}
void mi_trainer_erase_batch(Train_ResNet *t, Batch *b, int rank, int world) {
    MiCtx *c = ctx_of(t);
    if (!c->erase_on) return;
    const int n = b->n_images < t->batch_size ? b->n_images : t->batch_size;
    c->erase_rows = 0;
    if (mi_erase_plan(c->erase_seed, t->cur_epoch, t->cur_dump_id, rank, world, n, b->image_dim, c->erase_prob, c->erase_scale[0], c->erase_scale[1],
                      c->erase_ratio[0], c->erase_ratio[1], c->erase_last)) return;
    c->erase_rows = n;
    ck(mid_erase_batch(G.compute, b->images, n, (size_t)b->image_size, b->image_dim, c->erase_last, c->erase_fill.mode, c->erase_fill.value,
                       c->erase_fill.std, mi_erase_key(c->erase_seed, t->cur_epoch, t->cur_dump_id, rank, world), 0), "erase");
}
/* TrivialAugmentWide (resnet_mi.h, "TrivialAugmentWide") */
int mi_trainer_set_trivial_augment(Train_ResNet *t, int on, uint64_t seed) {
    MiCtx *c = ctx_of(t);
    if (!on) { c->ta_on = 0; c->ta_rows = 0; return 0; }
    const int dim = t->model->dims->input;
    if (mi_ta_plan(seed, 0, 0, 0, 1, 0, dim, NULL)) return -1; /* the argument rule (dim) is the plan's */
    if (!c->ta_last) c->ta_last = (MiTaRow *)calloc((size_t)t->batch_size, sizeof(MiTaRow));
    if (!c->ta_last) { mi_record_host_error("mi_trainer_set_trivial_augment", "no memory for the records"); return -1; }
    if (!c->ta_workspace) c->ta_workspace = mid_malloc(mid_ta_workspace_bytes(t->batch_size, dim));
    if (!c->ta_workspace) { mi_record_host_error("mi_trainer_set_trivial_augment", "no device memory for the workspace"); return -1; }
    c->ta_seed = seed;
    c->ta_rows = 0;
    c->ta_on = 1;
    return 0;
}
int mi_trainer_last_trivial_augment(const Train_ResNet *t, MiTaRow *out) {
    const MiCtx *c = ctx_of((Train_ResNet *)t);
    if (!c->ta_on || !out) { mi_record_host_error("mi_trainer_last_trivial_augment", "TrivialAugmentWide is off (mi_trainer_set_trivial_augment)"); return -1; }
    memcpy(out, c->ta_last, (size_t)c->ta_rows * sizeof(MiTaRow));
    return c->ta_rows;
}
void mi_trainer_ta_batch(Train_ResNet *t, Batch *b, int rank, int world) {
    MiCtx *c = ctx_of(t);
    if (!c->ta_on) return;
    const int n = b->n_images < t->batch_size ? b->n_images : t->batch_size;
    c->ta_rows = 0;
    if (b->image_dim != t->model->dims->input) { mi_record_host_error("mi_trainer_ta_batch", "the batch is not of the network's input size"); return; }
    if (mi_ta_plan(c->ta_seed, t->cur_epoch, t->cur_dump_id, rank, world, n, b->image_dim, c->ta_last)) return;
    c->ta_rows = n;
    ck(mid_trivial_augment(G.compute, b->images, n, (size_t)b->image_size, b->image_dim, (const mid_ta_row *)c->ta_last, c->ta_workspace), "trivial augment");
}
/* the two records (last, total) a loss head keeps on the device */
static int read_metrics(mid_loss_metrics *rec, MiLossMetrics *last, MiLossMetrics *total, int reset_total) {
    if (last) mid_memcpy_d2h(last, rec, sizeof *last, G.compute);
    if (total) mid_memcpy_d2h(total, rec + 1, sizeof *total, G.compute);
    if (reset_total) mid_memset(rec + 1, 0, sizeof(mid_loss_metrics), G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}
int mi_trainer_metrics(Train_ResNet *t, MiLossMetrics *last, MiLossMetrics *total, int reset_total) {
    return read_metrics(ctx_of(t)->loss_metrics, last, total, reset_total);
}

/* resnet.cu:3363-3383 */
float mi_host_loss(Train_ResNet *t, int *n_wrong) {
    const int N = t->batch_size, L = t->model->dims->output;
    if (ctx_of(t)->loss_flags & MI_LOSS_NO_PRED_COPY) { /* pred_cpu was not written: the device's record of this forward_pass */
        MiLossMetrics m = {0};
        mi_trainer_metrics(t, &m, NULL, 0);
        if (n_wrong) *n_wrong = (int)m.wrong_top1;
        return (float)m.loss_sum;
    }
    const float *pred = t->forward_buffer->pred_cpu;
    const int *lab = t->cur_batch->correct_classes_cpu;
    float loss = 0;
    int wrong = 0;
    for (int s = 0; s < N; s++) loss += -1 * logf(pred[(size_t)s * L + lab[s]]);
    for (int s = 0; s < N; s++) {
        const float pc = pred[(size_t)s * L + lab[s]];
        for (int cc = 0; cc < L; cc++)
            if (cc != lab[s] && pred[(size_t)s * L + cc] >= pc) { wrong++; break; }
    }
    if (n_wrong) *n_wrong = wrong;
    return loss;
}

/* ---------------------------------------------------------------------------------------------- */
/* Evaluation (resnet_mi.h): running statistics of every batch norm, the eval pass, its metrics. */
/* the device table of bn_running_update_kernel, one entry per unit: whenever the caches are rebuilt (build_buffers) or the sample count
 * changes (sync-BN) */
static void rs_build_table(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    if (!c->rs_arena) return;
    const int n = c->n_units;
    mid_bn_run_entry *tab = (mid_bn_run_entry *)malloc(sizeof(mid_bn_run_entry) * (size_t)n);
    const int64_t world = c->sync_bn && c->sync_bn_comm ? c->world : 1; /* sync-BN: the statistics are those of every replica's samples */
    for (int i = 0; i < n; i++) {
        const MiUnit *u = &c->units[i];
        const int64_t cnt = (int64_t)t->batch_size * u->bn->spatial_dim * u->bn->spatial_dim * world;
        tab[i].means = u->cache->means; tab[i].vars = u->cache->vars;
        tab[i].first = tab[i].off = u->rs_off; tab[i].C = u->bn->depth; tab[i].unbias = mi_bn_unbias(cnt);
    }
    mid_memcpy_h2d(c->rs_tab_dev, tab, sizeof(mid_bn_run_entry) * (size_t)n, G.compute);
    mid_stream_sync(G.compute);
    free(tab);
}
int mi_trainer_track_running_stats(Train_ResNet *t, int on, float momentum) {
    MiCtx *c = ctx_of(t);
    if (!on) { c->rs_on = 0; return 0; }
    if (!(momentum > 0.f && momentum <= 1.f)) { mi_record_host_error("mi_trainer_track_running_stats", "momentum lies in (0, 1]"); return -1; }
    if (!c->rs_arena) { /* the first time: means 0, variances 1, no update yet (switched off and on again, the values stay) */
        const MiUnit *lastu = &c->units[c->n_units - 1];
        const int n = c->n_units, sum = lastu->rs_off + lastu->bn->depth;
        c->rs_channels = sum; c->rs_updates = 0;
        c->rs_tab_dev = (mid_bn_run_entry *)mid_malloc(sizeof(mid_bn_run_entry) * (size_t)n);
        c->eval_row = (float *)mid_malloc(sizeof(float) * (size_t)t->batch_size);
        c->eval_rank = (int *)mid_malloc(sizeof(int) * (size_t)t->batch_size);
        c->eval_metrics = (mid_loss_metrics *)mid_malloc(2 * sizeof(mid_loss_metrics));
        float *one = (float *)malloc(sizeof(float) * (size_t)sum);
        for (int i = 0; i < sum; i++) one[i] = 1.f;
        c->rs_arena = (float *)mid_malloc(2 * sizeof(float) * (size_t)sum);
        if (!c->rs_tab_dev || !c->eval_row || !c->eval_rank || !c->eval_metrics || !c->rs_arena) {
            mi_record_host_error("mi_trainer_track_running_stats", "device allocation failed");
            mid_free(c->rs_tab_dev); mid_free(c->eval_row); mid_free(c->eval_rank); mid_free(c->eval_metrics); mid_free(c->rs_arena);
            c->rs_tab_dev = NULL; c->eval_row = NULL; c->eval_rank = NULL; c->eval_metrics = NULL; c->rs_arena = NULL;
            free(one);
            return -1;
        }
        mid_memset(c->rs_arena, 0, sizeof(float) * (size_t)sum, G.compute);
        mid_memcpy_h2d(c->rs_arena + sum, one, sizeof(float) * (size_t)sum, G.compute);
        mid_memset(c->eval_metrics, 0, 2 * sizeof(mid_loss_metrics), G.compute);
        mid_stream_sync(G.compute);
        free(one);
        rs_build_table(t);
    }
    c->rs_on = 1; c->rs_momentum = momentum;
    return 0;
}
int mi_trainer_running_stats_channels(const Train_ResNet *t) { return ((const MiCtx *)t->backend_ctx)->rs_channels; }
int64_t mi_trainer_running_updates(const Train_ResNet *t) { return ((const MiCtx *)t->backend_ctx)->rs_updates; }
int mi_trainer_get_running_stats(Train_ResNet *t, float *means, float *vars) {
    MiCtx *c = ctx_of(t);
    if (!c->rs_arena) { mi_record_host_error("mi_trainer_get_running_stats", "running statistics are not tracked (mi_trainer_track_running_stats)"); return -1; }
    const size_t b = sizeof(float) * (size_t)c->rs_channels;
    if (means) mid_memcpy_d2h(means, c->rs_arena, b, G.compute);
    if (vars) mid_memcpy_d2h(vars, c->rs_arena + c->rs_channels, b, G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}
int mi_trainer_set_running_stats(Train_ResNet *t, const float *means, const float *vars) {
    MiCtx *c = ctx_of(t);
    if (!c->rs_arena) { mi_record_host_error("mi_trainer_set_running_stats", "running statistics are not tracked (mi_trainer_track_running_stats)"); return -1; }
    if (!means || !vars) { mi_record_host_error("mi_trainer_set_running_stats", "means and vars are both needed"); return -1; }
    for (int i = 0; i < c->rs_channels; i++) {
        if (!isfinite(means[i]) || !isfinite(vars[i])) { mi_record_host_error("mi_trainer_set_running_stats", "a value is not finite"); return -1; }
        if (vars[i] < 0.f) { mi_record_host_error("mi_trainer_set_running_stats", "a variance is negative"); return -1; }
    }
    const size_t b = sizeof(float) * (size_t)c->rs_channels;
    mid_memcpy_h2d(c->rs_arena, means, b, G.compute);
    mid_memcpy_h2d(c->rs_arena + c->rs_channels, vars, b, G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}

static int eval_args_ok(const Train_ResNet *t, const char *who, int n_valid, int topk) {
    const MiCtx *c = (const MiCtx *)t->backend_ctx;
    if (!c->rs_on) { mi_record_host_error(who, "running statistics are not tracked (mi_trainer_track_running_stats)"); return -1; }
    if (c->policy == MI_STORE_FULL) { mi_record_host_error(who, "the eval pass does not run under the FULL store policy"); return -1; }
    if (n_valid < 1 || n_valid > t->batch_size) { mi_record_host_error(who, "n_valid lies in [1, batch_size]"); return -1; }
    if (topk < 1 || topk > t->model->dims->output) { mi_record_host_error(who, "topk lies in [1, number of classes]"); return -1; }
    return 0;
}
/* mi_trainer_eval_use_ema: the parameter arena <-> its averaged copy and the running arena <-> its averaged copy, in place on the compute
 * stream, in front of and behind the eval passes that score the averaged model.  The trunk re-lays the weights at its start, so it runs
 * on whatever the arena holds; the re-laid copies it leaves are the averaged model's, hence params_dirty.  Returns 1 where it exchanged */
static int ema_exchange(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    if (!c->ema_eval || !c->ema_arena) return 0;
    ck(mid_exchange(G.compute, mi_params_arena_base(t->model->params), c->ema_arena, c->arena_floats), "exchange (parameters)");
    ck(mid_exchange(G.compute, c->rs_arena, c->ema_rs, 2 * (size_t)c->rs_channels), "exchange (running statistics)");
    c->params_dirty = 1;
    return 1;
}
int mi_trainer_eval_forward(Train_ResNet *t, const float *images_dev, const int *labels_dev, int n_valid, int topk) {
    MiCtx *c = ctx_of(t);
    if (eval_args_ok(t, "mi_trainer_eval_forward", n_valid, topk)) return -1;
    if (!images_dev) { mi_record_host_error("mi_trainer_eval_forward", "no images"); return -1; }
    const Dims *d = t->model->dims;
    Activations *a = t->forward_buffer->activations;
    c->acts_from_eval = 1; /* the stored activations are no longer those of a forward_pass */
    const int swapped = !c->ema_swapped && ema_exchange(t);
    forward_trunk(t, images_dev, 1);
    if (swapped) ema_exchange(t); /* back: the head below reads logits only */
    /* the head over the valid rows only: pred, row losses and ranks, the eval records; no dlogits */
    if (labels_dev)
        ck(mid_loss_head(G.compute, a->linear_output, labels_dev, t->forward_buffer->pred, NULL, c->eval_row, c->eval_rank, n_valid, d->output, 0.f, topk,
                         c->eval_metrics, c->eval_metrics + 1), "loss head (eval)");
    else ck(mid_softmax(G.compute, a->linear_output, t->forward_buffer->pred, n_valid, d->output), "soft-max");
    return 0;
}
int mi_trainer_eval_metrics(Train_ResNet *t, MiLossMetrics *last, MiLossMetrics *total, int reset_total) {
    MiCtx *c = ctx_of(t);
    if (!c->eval_metrics) { mi_record_host_error("mi_trainer_eval_metrics", "running statistics are not tracked (mi_trainer_track_running_stats)"); return -1; }
    return read_metrics(c->eval_metrics, last, total, reset_total);
}
static void ev8_free(MiCtx *c) {
    mid_free(c->ev8_images); mid_free(c->ev8_bytes_dev); mid_free(c->ev8_labels_dev); mid_free(c->ev8_plan_dev);
    mid_free_host(c->ev8_bytes_pinned); mid_free_host(c->ev8_labels_pinned); mid_free_host(c->ev8_plan_pinned);
    c->ev8_images = NULL; c->ev8_bytes_dev = NULL; c->ev8_labels_dev = NULL; c->ev8_plan_dev = NULL;
    c->ev8_bytes_pinned = NULL; c->ev8_labels_pinned = NULL; c->ev8_plan_pinned = NULL; c->ev8_dim_in = 0;
}
/* resize 0: the centre crop through the decode kernel; else the whole image scaled to resize^2 (antialiased), the centre window of that */
static int eval_u8_batches(Train_ResNet *t, const uint8_t *images_host, const int *labels_host, int64_t n, int dim_in, int resize, int topk) {
    MiCtx *c = ctx_of(t);
    const int N = t->batch_size, D = t->model->dims->input;
    const size_t img = (size_t)dim_in * dim_in * 3, out_img = (size_t)D * D * 3;
    for (int64_t at = 0; at < n; at += N) {
        const int nv = n - at < N ? (int)(n - at) : N;
        if (at) mid_event_sync(c->ev8_copied); /* the pinned set is free again once the last batch's copies have left it */
        if (resize) for (int i = 0; i < nv; i++) { int *bx = c->ev8_plan_pinned + 5 * i; bx[0] = bx[1] = bx[4] = 0; bx[2] = bx[3] = dim_in; }
        else if (mi_augment_plan(MI_AUG_CENTER, 0, 0, 0, at, nv, dim_in, D, NULL, c->ev8_plan_pinned)) return -1;
        memcpy(c->ev8_bytes_pinned, images_host + (size_t)at * img, (size_t)nv * img);
        memcpy(c->ev8_labels_pinned, labels_host + at, (size_t)nv * sizeof(int));
        mid_memcpy_h2d(c->ev8_bytes_dev, c->ev8_bytes_pinned, (size_t)nv * img, G.compute);
        mid_memcpy_h2d(c->ev8_labels_dev, c->ev8_labels_pinned, (size_t)nv * sizeof(int), G.compute);
        mid_memcpy_h2d(c->ev8_plan_dev, c->ev8_plan_pinned, (size_t)nv * (resize ? 5 : 3) * sizeof(int), G.compute);
        mid_event_record(c->ev8_copied, G.compute);
        if (resize ? mid_resample_aa_u8(G.compute, c->ev8_bytes_dev, c->ev8_plan_dev, c->ev8_images, nv, dim_in, D, resize, (resize - D) / 2, (resize - D) / 2) :
            mid_decode_u8(G.compute, c->ev8_bytes_dev, c->ev8_plan_dev, c->ev8_images, nv, dim_in, D)) return -1;
        if (nv < N) mid_memset(c->ev8_images + (size_t)nv * out_img, 0, (size_t)(N - nv) * out_img * sizeof(float), G.compute);
        if (mi_trainer_eval_forward(t, c->ev8_images, c->ev8_labels_dev, nv, topk)) return -1;
    }
    return 0;
}
static int eval_u8(Train_ResNet *t, const char *who, const uint8_t *images_host, const int *labels_host, int64_t n, int dim_in, int resize, int topk,
                   MiLossMetrics *out) {
    MiCtx *c = ctx_of(t);
    const int N = t->batch_size, D = t->model->dims->input;
    if (eval_args_ok(t, who, 1, topk)) return -1;
    if (!images_host || !labels_host || n < 1) { mi_record_host_error(who, "images, labels and n >= 1 are needed"); return -1; }
    if (!resize && dim_in < D) { mi_record_host_error(who, "dim_in is smaller than the network's input"); return -1; }
    if (dim_in < 1) { mi_record_host_error(who, "dim_in >= 1 is needed"); return -1; }
    const size_t img = (size_t)dim_in * dim_in * 3, out_img = (size_t)D * D * 3;
    if (c->ev8_dim_in != dim_in) {
        mid_device_sync();
        ev8_free(c);
        c->ev8_images = (float *)mid_malloc((size_t)N * out_img * sizeof(float));
        c->ev8_bytes_dev = (uint8_t *)mid_malloc((size_t)N * img);
        c->ev8_labels_dev = (int *)mid_malloc((size_t)N * sizeof(int));
        c->ev8_plan_dev = (int *)mid_malloc((size_t)N * 5 * sizeof(int)); /* a box plan at most */
        c->ev8_bytes_pinned = (uint8_t *)mid_malloc_host((size_t)N * img);
        c->ev8_labels_pinned = (int *)mid_malloc_host((size_t)N * sizeof(int));
        c->ev8_plan_pinned = (int *)mid_malloc_host((size_t)N * 5 * sizeof(int));
        if (!c->ev8_images || !c->ev8_bytes_dev || !c->ev8_labels_dev || !c->ev8_plan_dev || !c->ev8_bytes_pinned || !c->ev8_labels_pinned ||
            !c->ev8_plan_pinned) { ev8_free(c); mi_record_host_error(who, "allocation of the staging buffers failed"); return -1; }
        if (!c->ev8_copied) c->ev8_copied = mid_event_create();
        c->ev8_dim_in = dim_in;
    }
    mid_memset(c->eval_metrics + 1, 0, sizeof(mid_loss_metrics), G.compute);
    c->ema_swapped = ema_exchange(t); /* the averaged model: one exchange around the whole loop, not one per batch */
    const int rc = eval_u8_batches(t, images_host, labels_host, n, dim_in, resize, topk);
    if (c->ema_swapped) { c->ema_swapped = 0; ema_exchange(t); }
    if (rc) return -1;
    MiLossMetrics total;
    if (mi_trainer_eval_metrics(t, NULL, &total, 0)) return -1; /* the one synchronise */
    if (out) *out = total;
    return 0;
}
int mi_trainer_eval_u8(Train_ResNet *t, const uint8_t *images_host, const int *labels_host, int64_t n, int dim_in, int topk, MiLossMetrics *out) {
    return eval_u8(t, "mi_trainer_eval_u8", images_host, labels_host, n, dim_in, 0, topk, out);
}
int mi_trainer_eval_u8_resized(Train_ResNet *t, const uint8_t *images_host, const int *labels_host, int64_t n, int dim_in, int resize, int topk,
                               MiLossMetrics *out) {
    if (resize < t->model->dims->input) { mi_record_host_error("mi_trainer_eval_u8_resized", "resize is smaller than the network's input"); return -1; }
    return eval_u8(t, "mi_trainer_eval_u8_resized", images_host, labels_host, n, dim_in, resize, topk, out);
}

/* ---------------------------------------------------------------------------------------------- */
/* Weight averaging (resnet_mi.h): an EMA of the parameter arena and of the running-statistics arena. */
static void ema_snapshot(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    mid_memcpy_d2d(c->ema_arena, mi_params_arena_base(t->model->params), c->arena_floats * sizeof(float), G.compute);
    mid_memcpy_d2d(c->ema_rs, c->rs_arena, 2 * sizeof(float) * (size_t)c->rs_channels, G.compute);
    mid_stream_sync(G.compute);
    c->ema_updates = 0;
}
int mi_trainer_set_ema(Train_ResNet *t, double decay, int every, int warmup) {
    MiCtx *c = ctx_of(t);
    const char *who = "mi_trainer_set_ema";
    if (!c->rs_arena) { mi_record_host_error(who, "running statistics were never tracked (mi_trainer_track_running_stats): an averaged model could not be evaluated"); return -1; }
    if (!(decay >= 0.0 && decay < 1.0)) { mi_record_host_error(who, "decay lies in [0, 1)"); return -1; }
    if (every < 0) { mi_record_host_error(who, "every is >= 0 (0: no updates)"); return -1; }
    if (!c->ema_arena) { /* the first time: both arenas, a copy of the current values, no update yet */
        float *pa = (float *)mid_malloc(c->arena_floats * sizeof(float)), *rs = (float *)mid_malloc(2 * sizeof(float) * (size_t)c->rs_channels);
        if (!pa || !rs) { mid_free(pa); mid_free(rs); mi_record_host_error(who, "device allocation failed"); return -1; }
        c->ema_arena = pa; c->ema_rs = rs;
        ema_snapshot(t);
    }
    c->ema_decay = decay; c->ema_every = every; c->ema_warmup = warmup != 0;
    return 0;
}
static int ema_ready(const MiCtx *c, const char *who) {
    if (c->ema_arena) return 1;
    mi_record_host_error(who, "no averaged model (mi_trainer_set_ema)");
    return 0;
}
int mi_trainer_ema_reset(Train_ResNet *t) {
    if (!ema_ready(ctx_of(t), "mi_trainer_ema_reset")) return -1;
    ema_snapshot(t);
    return mid_last_error()[0] ? -1 : 0;
}
int64_t mi_trainer_ema_updates(const Train_ResNet *t) { return ((const MiCtx *)t->backend_ctx)->ema_updates; }
int mi_trainer_eval_use_ema(Train_ResNet *t, int on) {
    MiCtx *c = ctx_of(t);
    if (!ema_ready(c, "mi_trainer_eval_use_ema")) return -1;
    c->ema_eval = on != 0;
    return 0;
}
static int ema_location_ok(const MiCtx *c, const char *who, int i, const void *host) {
    if (!ema_ready(c, who)) return 0;
    if (i < 0 || i >= c->n_loc) { mi_record_host_error(who, "no such location"); return 0; }
    if (!host) { mi_record_host_error(who, "no host array"); return 0; }
    return 1;
}
int mi_trainer_ema_get_location(Train_ResNet *t, int i, float *host) {
    MiCtx *c = ctx_of(t);
    if (!ema_location_ok(c, "mi_trainer_ema_get_location", i, host)) return -1;
    mid_memcpy_d2h(host, c->ema_arena + c->loc_off[i], sizeof(float) * (size_t)t->model->params->sizes[i], G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}
int mi_trainer_ema_set_location(Train_ResNet *t, int i, const float *host) {
    MiCtx *c = ctx_of(t);
    const char *who = "mi_trainer_ema_set_location";
    if (!ema_location_ok(c, who, i, host)) return -1;
    const size_t n = (size_t)t->model->params->sizes[i];
    for (size_t j = 0; j < n; j++) if (!isfinite(host[j])) { mi_record_host_error(who, "a value is not finite"); return -1; }
    mid_memcpy_h2d(c->ema_arena + c->loc_off[i], host, sizeof(float) * n, G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}
int mi_trainer_ema_get_running_stats(Train_ResNet *t, float *means, float *vars) {
    MiCtx *c = ctx_of(t);
    if (!ema_ready(c, "mi_trainer_ema_get_running_stats")) return -1;
    const size_t b = sizeof(float) * (size_t)c->rs_channels;
    if (means) mid_memcpy_d2h(means, c->ema_rs, b, G.compute);
    if (vars) mid_memcpy_d2h(vars, c->ema_rs + c->rs_channels, b, G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}
int mi_trainer_ema_set_running_stats(Train_ResNet *t, const float *means, const float *vars) {
    MiCtx *c = ctx_of(t);
    const char *who = "mi_trainer_ema_set_running_stats";
    if (!ema_ready(c, who)) return -1;
    if (!means || !vars) { mi_record_host_error(who, "means and vars are both needed"); return -1; }
    for (int i = 0; i < c->rs_channels; i++) {
        if (!isfinite(means[i]) || !isfinite(vars[i])) { mi_record_host_error(who, "a value is not finite"); return -1; }
        if (vars[i] < 0.f) { mi_record_host_error(who, "a variance is negative"); return -1; }
    }
    const size_t b = sizeof(float) * (size_t)c->rs_channels;
    mid_memcpy_h2d(c->ema_rs, means, b, G.compute);
    mid_memcpy_h2d(c->ema_rs + c->rs_channels, vars, b, G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}
int mi_trainer_ema_restore(Train_ResNet *t, const float *params_arena_host, const float *stats_host, int64_t updates) {
    MiCtx *c = ctx_of(t);
    if (!ema_ready(c, "mi_trainer_ema_restore")) return -1;
    mid_memcpy_h2d(c->ema_arena, params_arena_host, c->arena_floats * sizeof(float), G.compute);
    mid_memcpy_h2d(c->ema_rs, stats_host, 2 * sizeof(float) * (size_t)c->rs_channels, G.compute);
    mid_stream_sync(G.compute);
    c->ema_updates = updates;
    return mid_last_error()[0] ? -1 : 0;
}

/* BN' (+fused ReLU') then conv' : prepareAndDoActivationAndBatchNormDeriv + prepreAndDoConvolutionDeriv */
/* the aux stream must have finished the previous weight gradient before a dgrad may overwrite the rolling buffer it reads */
static void join_wgrad(MiCtx *c) {
    if (c->wgrad_pending) { mid_stream_wait_event(G.compute, c->ev_wgrad_done); c->wgrad_pending = 0; }
}
/* mode 2: next slot of the derivative ring; the compute stream first waits for the weight gradient (if any) that still
 * reads the slot's previous contents */
static float *ring_take(MiCtx *c, int *slot) {
    const int i = c->ring_next;
    c->ring_next = (i + 1) % MI_RING;
    if (c->ring_busy[i]) { mid_stream_wait_event(G.compute, c->ring_ev[i]); c->ring_busy[i] = 0; }
    if (slot) *slot = i;
    return c->ring_buf[i];
}
/* d_slot: ring slot holding d_conv_out (mode 2), -1 otherwise.  fz: the BN'-partials hand-off between a fusing dgrad and the next
 * unit (nparts > 0: this unit's BN' reduction is done); fz_req: what this unit's dgrad is to fill it with, or NULL (unit_fz_request) */
static void unit_bwd(Train_ResNet *t, MiUnit *u, const float *dy, const float *mask_src, int mask_mode, float *gated_out, float *d_conv_out,
                     int d_slot, float *dx, const float *addend, mid_bn_bwd_parts *fz, const mid_bn_bwd_parts *fz_req) {
    MiCtx *c = ctx_of(t);
    MiLayer *L = &u->L;
    const float *in = u->in ? u->in : t->cur_batch->images;
    const int Ho = L->H / L->stride;
    /* BN' of this unit (HBM-bound) runs next to earlier units' weight gradients (FMA-bound, low-priority aux stream);
     * mask_mode 3: ReLU' of the block output fused in, and its product with the upstream gradient kept (gated_out) */
    ck(mi_bn_bwd_unit(&c->lw, G.compute, fz, u->conv_out, L->out_dt, u->bn->gamma, u->bn->beta, u->cache->means, u->cache->vars, dy, mask_src,
                      mask_mode, gated_out, c->dtype, d_conv_out, u->dbn->gamma, u->dbn->beta, t->batch_size, L->K, Ho * Ho, t->eps), "batch norm backward");
    /* the channel-last copy of d_conv_out that the channel-last dgrad AND the weight gradient read: made here, before either is
     * launched, so that every weight-gradient schedule (the free-running one starts before the dgrad) runs the same kernels */
    ck(mi_layer_dy_relayout(L, G.compute, d_conv_out), "dY re-layout (channel-last)");
    if (c->overlap_wgrad == 2 && d_slot >= 0) {
        /* d_conv_out is final once BN' is: the weight gradient may start now and run for as long as the slot lives */
        mid_event_record(c->ev_bn_done, G.compute);
        mid_stream_wait_event(G.aux, c->ev_bn_done);
        ck(mi_layer_wgrad(L, &c->lw, G.aux, in, d_conv_out, u->dw), "convolution wgrad");
        mid_event_record(c->ring_ev[d_slot], G.aux);
        c->ring_busy[d_slot] = 1;
        mid_event_record(c->ev_wgrad_done, G.aux);
        c->wgrad_pending = 1;
        if (dx) ck(mi_layer_dgrad(L, &c->lw, G.compute, d_conv_out, dx, addend, fz_req, fz), "convolution dgrad");
        return;
    }
    join_wgrad(c);
    if (dx) ck(mi_layer_dgrad(L, &c->lw, G.compute, d_conv_out, dx, addend, fz_req, fz), "convolution dgrad");
    if (c->overlap_wgrad) {
        mid_event_record(c->ev_bn_done, G.compute);
        mid_stream_wait_event(G.aux, c->ev_bn_done);
        ck(mi_layer_wgrad(L, &c->lw, G.aux, in, d_conv_out, u->dw), "convolution wgrad");
        mid_event_record(c->ev_wgrad_done, G.aux);
        c->wgrad_pending = 1;
    } else ck(mi_layer_wgrad(L, &c->lw, G.compute, in, d_conv_out, u->dw), "convolution wgrad");
}
/* the request for u's fusing dgrad: the reduction pass of the BN' of the unit that made u's input (mi_layer_fz_request) */
static const mid_bn_bwd_parts *unit_fz_request(MiCtx *c, const MiUnit *u, const MiUnit *producer, mid_bn_bwd_parts *req) {
    return mi_layer_fz_request(&u->L, &c->lw, req, producer->conv_out, producer->out, producer->cache->means);
}
/* RECOMPUTE_BN: relu(BN(conv_out)) of a unit, re-derived into the scratch the unit behind it reads (resnet_clean.cu:2714, :2753) */
static void unit_recompute(Train_ResNet *t, const MiUnit *u) {
    MiCtx *c = ctx_of(t);
    const int Ho = u->L.H / u->L.stride;
    ck(mid_bn_apply_t(G.compute, u->conv_out, c->dtype, u->bn->gamma, u->bn->beta, NULL, u->cache->means, u->cache->vars, u->act_out, c->dtype,
                      t->batch_size, u->L.K, Ho * Ho, t->eps, 1, NULL, 0), "BN recompute");
}
/* resnet.cu:1777-2248 */
void backwards_pass(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    const Dims *d = t->model->dims;
    const Params *p = t->model->params;
    Activations *a = t->forward_buffer->activations;
    Backprop_Buffer *bb = t->backprop_buffer;
    const Params *dp = bb->param_derivs;
    Activations *da = bb->activation_derivs;
    const int N = t->batch_size, L = d->output, D = d->final_depth, nb = d->n_conv_blocks;
    const int recompute = c->policy == MI_STORE_RECOMPUTE_BN;
    if (c->acts_from_eval) { /* the stored activations are an eval pass's (running statistics): no gradient of any loss */
        mi_record_host_error("backwards_pass", "the last pass was mi_trainer_eval_forward: run forward_pass first");
        return;
    }
    mid_event_record(c->ev_t[2], G.compute);
    bind_sync_bn(c);
    if (weights_stale(c)) relayout_weights(c); /* parameters were rewritten from the host after forward_pass */
    c->dp_cursor = c->arena_floats;
    c->n_buckets = 0;
    /* dlogits = softmax - onehot, batch SUM (no 1/N: resnet.cu:1806-1811) */
    if (!(c->loss_flags & MI_LOSS_DEVICE)) /* (the loss head of forward_pass left it) */
        ck(mid_ce_deriv(G.compute, t->forward_buffer->pred, t->cur_batch->correct_classes, bb->output_layer_deriv, N, L), "cross-entropy derivative");
    /* FC: dW = pooled^T dlogits (:1823), dpooled = dlogits W^T (:1830) -- no transposed temporaries */
    ck(mid_gemm_tn(G.compute, a->final_conv_output_pooled, bb->output_layer_deriv, dp->fully_connected, D, N, L), "FC wgrad");
    ck(mid_gemm_nt(G.compute, bb->output_layer_deriv, p->fully_connected, da->final_conv_output_pooled, N, L, D), "FC dgrad");
    mi_dp_reduce_ready(t, (size_t)(dp->fully_connected - c->g_arena), 0);
    const ConvBlock *last = p->conv_blocks[nb - 1];
    const int Hl = last->incoming_spatial_dim;
    ck(mid_avgpool_bwd_t(G.compute, da->final_conv_output_pooled, da->activation_conv_blocks[nb - 1]->output_activated, c->dtype, N, D, Hl * Hl),
       "average pool backward");
    const int ring = c->overlap_wgrad == 2;
    mid_bn_bwd_parts fz = {NULL}, req; /* BN'-partials hand-off from a fusing dgrad to the next unit (unit_bwd) */
    for (int i = nb - 1; i >= 0; i--) {
        MiUnit *red = unit_of(c, i, MI_U_RED), *spa = unit_of(c, i, MI_U_SPA), *expa = unit_of(c, i, MI_U_EXP), *proj = unit_of(c, i, MI_U_PROJ);
        const MiUnit *below = i == 0 ? NULL : unit_of(c, i - 1, MI_U_EXP); /* the unit that made this block's input */
        Activation_ConvBlock *dk = da->activation_conv_blocks[i];
        float *dbin = i == 0 ? da->init_convblock_input : da->activation_conv_blocks[i - 1]->output_activated;
        const float *up = dk->output_activated; /* dL/d(block output) */
        const float *exp_dy, *exp_mask, *red_addend;
        int exp_mode, s_proj = -1, s_exp = -1, s_spa = -1, s_red = -1;
        if (ring) { /* this block's derivative tensors: fresh ring slots (resnet_cudnn_lowmem.cu:2152-2170 keeps four) */
            dk->output = ring_take(c, NULL);
            if (proj) dk->transformed_residual = ring_take(c, &s_proj);
        }
        const int up_gated = fz.nparts > 0; /* the block above's reduction dgrad already gated `up` by this block's output and summed for the expansion BN' */
        if (proj) {
            /* ReLU' of the block output (doActivationDeriv, :1934) is fused into the projection BN' as an external mask; that
             * pass also leaves relu'(out) * up in dk->output, which the expansion BN' then reads instead of up + mask */
            unit_bwd(t, proj, up, expa->out, 3, dk->output, dk->transformed_residual, s_proj, dbin, NULL, &fz, NULL);
            exp_dy = dk->output; exp_mask = NULL; exp_mode = 0;
            red_addend = dbin; /* reduce-conv dgrad accumulates onto the projection path (toAdd, :2157) */
        } else {
            /* doActivationDeriv (:1934) rides in the expansion BN' reduce pass, which also leaves relu'(out) * up in dk->output
             * (one pass over the block output less than a separate ReLU' kernel) */
            exp_dy = up; exp_mask = expa->out; exp_mode = 3;
            red_addend = up_gated ? up : dk->output; /* identity shortcut: setVal 0 + addVec (:2003-2004) folded into the dgrad epilogue */
        }
        if (ring) { dk->post_expanded = ring_take(c, &s_exp); dk->post_spatial_activated = ring_take(c, NULL); }
        if (recompute) unit_recompute(t, spa); /* the expansion's input */
        unit_bwd(t, expa, exp_dy, exp_mask, exp_mode, dk->output, dk->post_expanded, s_exp, dk->post_spatial_activated, NULL, &fz,
                 unit_fz_request(c, expa, spa, &req));
        /* the call resnet.cu:2060-2083 forgot; present in resnet_cudnn.cu:2365-2366 */
        if (ring) { dk->post_spatial = ring_take(c, &s_spa); dk->post_reduced_activated = ring_take(c, NULL); }
        if (recompute) unit_recompute(t, red); /* the 3x3's input */
        unit_bwd(t, spa, dk->post_spatial_activated, NULL, 1, NULL, dk->post_spatial, s_spa, dk->post_reduced_activated, NULL, &fz,
                 unit_fz_request(c, spa, red, &req));
        if (ring) dk->post_reduced = ring_take(c, &s_red);
        unit_bwd(t, red, dk->post_reduced_activated, NULL, 1, NULL, dk->post_reduced, s_red, dbin, red_addend, &fz,
                 below ? unit_fz_request(c, red, below, &req) : NULL);
        mi_dp_reduce_ready(t, (size_t)(red->dw - c->g_arena), 0);
    }
    const int Hs = d->input / d->init_conv_stride;
    int s_stem = -1;
    if (ring) { da->init_conv_activated = ring_take(c, NULL); da->init_conv_applied = ring_take(c, &s_stem); }
    ck(mid_maxpool_bwd_t(G.compute, a->max_inds, da->init_convblock_input, da->init_conv_activated, c->dtype, N, d->init_conv_filters, Hs,
                         d->init_maxpool_dim, d->init_maxpool_stride), "max-pool backward");
    unit_bwd(t, unit_of(c, -1, MI_U_STEM), da->init_conv_activated, NULL, 1, NULL, da->init_conv_applied, s_stem, NULL, NULL, &fz, NULL);
    mi_dp_reduce_ready(t, 0, 1);
    mid_event_record(c->ev_t[3], G.compute);
}

/* Where the data-parallel path may cut the gradient arena: after the FC layer, after each block (walking backwards) and at
 * the end of backward.  A bucket is emitted at a cut as soon as at least bucket_bytes are pending.  Pure arithmetic on the
 * arena offsets (the carve order of build_params), shared by backwards_pass and mi_debug_dp_plan. */
int mi_dp_plan_buckets(const Dims *d, size_t bucket_bytes, size_t *from, size_t *to, int max) {
    size_t arena;
    (void)count_locations(d, &arena);
    /* offsets of each block's first tensor and of the FC tensor */
    size_t *boff = (size_t *)malloc(sizeof(size_t) * (size_t)(d->n_conv_blocks + 1));
    int inc = d->init_conv_filters, ex = 4 * inc, red = inc;
    size_t off = align_up((size_t)d->init_kernel_dim * d->init_kernel_dim * inc * 3) + 2 * align_up(inc);
    for (int i = 0; i < d->n_conv_blocks; i++) {
        int stride = 1;
        if (d->is_block_spatial_reduction[i] == 1) { stride = 2; red *= 2; ex *= 2; }
        boff[i] = off;
        off += align_up((size_t)inc * red) + align_up((size_t)red * red * 9) + align_up((size_t)ex * red) + 4 * align_up(red) + 2 * align_up(ex);
        if (inc != ex) off += align_up((size_t)inc * ex * (stride == 2 ? 9 : 1)) + 2 * align_up(ex);
        inc = ex;
    }
    const size_t fc_off = off;
    int n = 0;
    size_t cursor = arena;
    /* at most MI_MAX_BUCKETS buckets (one event each): the last slot is kept for the forced final cut, so a network with more
     * cut points than slots gets a larger last bucket, never a lost range */
#define CUT(from_, force_)                                                                      \
    do {                                                                                        \
        if ((from_) < cursor && ((force_) || ((cursor - (from_)) * sizeof(float) >= bucket_bytes && n < MI_MAX_BUCKETS - 1))) { \
            if (n < max) { from[n] = (from_); to[n] = cursor; }                                  \
            n++; cursor = (from_);                                                              \
        }                                                                                       \
    } while (0)
    CUT(fc_off, 0);
    for (int i = d->n_conv_blocks - 1; i >= 0; i--) CUT(boff[i], 0);
    CUT((size_t)0, 1);
#undef CUT
    free(boff);
    return n;
}

/* Gradient accumulation (resnet_mi.h): k micro-batches per optimizer update.  A backward pass overwrites the gradient arena, so the
 * window's sum lives in an arena of its own: the first k - 1 update_parameters of a window only add the gradient arena into it
 * (acc_pending counts them), the k-th folds it back -- g = (acc + g) * scale -- in front of the unchanged optimizer path. */
static int acc_collecting(const MiCtx *c) { return c->acc_k > 1 && c->acc_pending + 1 < c->acc_k; }
int mi_trainer_set_accumulation(Train_ResNet *t, int k, float scale) {
    MiCtx *c = ctx_of(t);
    const char *who = "mi_trainer_set_accumulation";
    if (k < 1) { mi_record_host_error(who, "k is >= 1 (1: no accumulation)"); return -1; }
    if (!(scale > 0.f) || isinf(scale)) { mi_record_host_error(who, "scale is finite and > 0"); return -1; }
    if (c->acc_pending > 0) { mi_record_host_error(who, "a window is open: micro-batches are pending"); return -1; }
    if (c->acc_in_step) { mi_record_host_error(who, "not between forward_pass and update_parameters"); return -1; }
    if (k > 1 && !c->acc_arena) { /* the first time: the arena, through the allocator every tensor comes from */
        c->acc_arena = (float *)mid_malloc(c->arena_floats * sizeof(float));
        if (!c->acc_arena) { mi_record_host_error(who, "device allocation failed"); return -1; }
    }
    c->acc_k = k; c->acc_scale = scale;
    return 0;
}
int mi_trainer_accumulation(const Train_ResNet *t, int *k, int *pending) {
    const MiCtx *c = (const MiCtx *)t->backend_ctx;
    if (k) *k = c->acc_k;
    if (pending) *pending = c->acc_pending;
    return 0;
}
float *mi_debug_accum_arena(const Train_ResNet *t) { return ((const MiCtx *)t->backend_ctx)->acc_arena; }
int mi_trainer_accum_restore(Train_ResNet *t, const float *arena_host, int pending) {
    MiCtx *c = ctx_of(t);
    if (!c->acc_arena || pending < 0 || pending >= c->acc_k) return -1;
    if (pending) {
        mid_memcpy_h2d(c->acc_arena, arena_host, c->arena_floats * sizeof(float), G.compute);
        mid_stream_sync(G.compute);
    }
    c->acc_pending = pending;
    return mid_last_error()[0] ? -1 : 0;
}

/* data parallel: hand the finished tail [from, cursor) of the gradient arena to RCCL on the comm stream as soon
 * as it is at least one bucket (or `force`).  Gradients become ready FC-first, i.e. from the arena's end
 * (the order update_parameters walks, resnet.cu:2952). */
void mi_dp_reduce_ready(Train_ResNet *t, size_t from, int force) {
    MiCtx *c = ctx_of(t);
    const int pending = c->wgrad_pending;
    if (force) join_wgrad(c); /* end of backward: every weight gradient is on the compute stream's timeline */
    if (!c->comm) return;
    if (acc_collecting(c)) return; /* this micro-batch's gradients are summed on this rank: no bucket, no collective */
    if (from >= c->dp_cursor) return;
    const size_t n = c->dp_cursor - from;
    if (!force && n * sizeof(float) < c->bucket_bytes) return;
    if (!force && c->n_buckets >= MI_MAX_BUCKETS - 1) return; /* the last event slot is kept for the forced final cut (mi_dp_plan_buckets) */
    mid_event_record(c->ev_grads, G.compute);
    mid_stream_wait_event(G.comm, c->ev_grads);
    /* the bucket also holds weight gradients from the aux stream: the comm stream waits for the latest of them itself,
     * the compute stream does not stall */
    if (pending) mid_stream_wait_event(G.comm, c->ev_wgrad_done);
    if (c->acc_k > 1) { /* the window's last micro-batch: the bucket's sum, scaled on this rank, is what is reduced */
        ck(mid_grad_accumulate(G.comm, c->acc_arena + from, c->g_arena + from, c->dp_cursor - from, MID_ACC_FOLD, c->acc_scale), "gradient fold (bucket)");
        c->acc_folded = 1;
    }
    ck(mid_rccl_allreduce_sum(c->comm, c->g_arena + from, c->dp_cursor - from, G.comm), "RCCL all-reduce");
    const int b = c->n_buckets++; /* < MI_MAX_BUCKETS by the rule above */
    c->bk_from[b] = from; c->bk_to[b] = c->dp_cursor;
    mid_event_record(c->bk_ev[b], G.comm);
    c->dp_cursor = from;
    c->dp_pending = 1;
}

/* ---- momentum SGD / LARS, gradient clipping (kernels_optim.hip) ---- */
/* The chunk table of n tensors (tensor i: sizes[i] floats at float offset off[i], off holds n + 1 entries): chunks of at most
 * MID_OPT_CHUNK floats that never cross a tensor, so no padding word between tensors is in one.  first_chunk: n + 1 entries, the
 * last the number of chunks.  Returns the table (malloc; one unused entry where there is no chunk), or NULL with mi_last_error set
 * under `who`: host arithmetic only */
static mid_chunk *cut_chunks(const char *who, const size_t *off, const int *sizes, int n, int *first_chunk) {
    if (n < 1) { mi_record_host_error(who, "no tensors"); return NULL; }
    size_t n_chunks = 0;
    for (int i = 0; i < n; i++) {
        if (off[i] % 4 || off[i + 1] < off[i] + (size_t)sizes[i] || sizes[i] < 0 || off[i] + (size_t)sizes[i] > (size_t)INT32_MAX) {
            mi_record_host_error(who, "tensor offsets must ascend in multiples of 4 floats below 2^31, each tensor within its gap");
            return NULL;
        }
        n_chunks += ((size_t)sizes[i] + MID_OPT_CHUNK - 1) / MID_OPT_CHUNK;
    }
    mid_chunk *ch = (mid_chunk *)malloc(sizeof(mid_chunk) * (n_chunks ? n_chunks : 1));
    int k = 0;
    for (int i = 0; i < n; i++) {
        first_chunk[i] = k;
        for (int s0 = 0; s0 < sizes[i]; s0 += MID_OPT_CHUNK) {
            ch[k].tensor = i; ch[k].start = (int)(off[i] + (size_t)s0);
            ch[k].len = sizes[i] - s0 < MID_OPT_CHUNK ? sizes[i] - s0 : MID_OPT_CHUNK;
            ch[k].pad = 0;
            k++;
        }
    }
    first_chunk[n] = k;
    return ch;
}

int mi_clip_init(MiClip *k, const char *who, const size_t *off, const int *sizes, int n) {
    memset(k, 0, sizeof *k);
    int *first = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n + 1 : 1));
    mid_chunk *ch = cut_chunks(who, off, sizes, n, first);
    if (!ch) { free(first); return -1; }
    const size_t nc = (size_t)first[n];
    free(first);
    k->n_chunks = (int)nc;
    const size_t bytes[3] = {sizeof(mid_chunk) * (nc ? nc : 1), sizeof(double) * (nc ? nc : 1), sizeof(mid_clip_record)};
    k->chunks_dev = (mid_chunk *)mid_malloc(bytes[0]);
    k->part_dev = (double *)mid_malloc(bytes[1]);
    k->rec_dev = (mid_clip_record *)mid_malloc(bytes[2]);
    k->bytes = bytes[0] + bytes[1] + bytes[2];
    int rc = 0;
    if (!k->chunks_dev || !k->part_dev || !k->rec_dev) { mi_record_host_error(who, "device allocation failed"); rc = -1; }
    else {
        MiGlobal *g = mi_global();
        if (nc) mid_memcpy_h2d(k->chunks_dev, ch, sizeof(mid_chunk) * nc, g->compute);
        mid_memset(k->rec_dev, 0, sizeof(mid_clip_record), g->compute);
        mid_stream_sync(g->compute);
    }
    free(ch);
    if (rc) mi_clip_free(k);
    return rc;
}
void mi_clip_free(MiClip *k) {
    mid_free(k->chunks_dev); mid_free(k->part_dev); mid_free(k->rec_dev);
    memset(k, 0, sizeof *k);
}
int mi_clip_run(const MiClip *k, mid_stream s, float *g, float max_norm) {
    if (mid_clip_norm(s, g, k->chunks_dev, k->n_chunks, k->part_dev)) return -1;
    if (mid_clip_coef(s, k->part_dev, k->n_chunks, max_norm, k->rec_dev)) return -1;
    return mid_clip_scale(s, g, k->chunks_dev, k->n_chunks, k->rec_dev);
}

int mi_optim_init(MiOptim *o, int kind, float momentum, float trust_coef, const size_t *off, const int *sizes, const int *is_weight, int n) {
    memset(o, 0, sizeof *o);
    o->kind = kind; o->momentum = momentum; o->trust_coef = trust_coef;
    if (kind == MI_OPT_ADAM) return 0;
    if (kind != MI_OPT_SGD && kind != MI_OPT_LARS) { mi_record_host_error("mi_optim_init", "unknown optimizer kind"); return -1; }
    o->first_chunk = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n + 1 : 1));
    mid_chunk *ch = cut_chunks("mi_optim_init", off, sizes, n, o->first_chunk);
    if (!ch) { free(o->first_chunk); o->first_chunk = NULL; return -1; }
    int *isw = (int *)malloc(sizeof(int) * (size_t)n);
    o->off = (size_t *)malloc(sizeof(size_t) * (size_t)(n + 1));
    for (int i = 0; i < n; i++) {
        o->off[i] = off[i];
        isw[i] = is_weight[i] != 0;
    }
    o->off[n] = off[n];
    const int k = o->first_chunk[n];
    o->n_tensors = n; o->n_chunks = k;
    o->chunks_dev = (mid_chunk *)mid_malloc(sizeof(mid_chunk) * (size_t)(k ? k : 1));
    o->first_chunk_dev = (int *)mid_malloc(sizeof(int) * (size_t)(n + 1));
    o->is_weight_dev = (int *)mid_malloc(sizeof(int) * (size_t)n);
    o->part_dev = (double *)mid_malloc(2 * sizeof(double) * (size_t)(k ? k : 1));
    o->sq_dev = (double *)mid_malloc(2 * sizeof(double) * (size_t)n);
    o->trust_dev = (float *)mid_malloc(sizeof(float) * (size_t)n);
    int rc = 0;
    if (!o->chunks_dev || !o->first_chunk_dev || !o->is_weight_dev || !o->part_dev || !o->sq_dev || !o->trust_dev) rc = -1;
    else {
        MiGlobal *g = mi_global();
        if (k) mid_memcpy_h2d(o->chunks_dev, ch, sizeof(mid_chunk) * (size_t)k, g->compute);
        mid_memcpy_h2d(o->first_chunk_dev, o->first_chunk, sizeof(int) * (size_t)(n + 1), g->compute);
        mid_memcpy_h2d(o->is_weight_dev, isw, sizeof(int) * (size_t)n, g->compute);
        mid_memset(o->sq_dev, 0, 2 * sizeof(double) * (size_t)n, g->compute);
        mid_stream_sync(g->compute);
    }
    free(ch); free(isw);
    if (rc) mi_optim_free(o);
    return rc;
}
void mi_optim_free(MiOptim *o) {
    mid_free(o->chunks_dev); mid_free(o->first_chunk_dev); mid_free(o->is_weight_dev);
    mid_free(o->part_dev); mid_free(o->sq_dev); mid_free(o->trust_dev);
    free(o->off); free(o->first_chunk);
    memset(o, 0, sizeof *o);
}
/* first tensor whose start is >= pos */
static int optim_tensor_at(const MiOptim *o, size_t pos) {
    int lo = 0, hi = o->n_tensors;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (o->off[mid] < pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}
int mi_optim_step(const MiOptim *o, mid_stream s, float *p, float *g, float *b, size_t from, size_t to, float lr, float wd, float wd_norm,
                  int *nan_flag, int want_norms) {
    const int t0 = optim_tensor_at(o, from), t1 = optim_tensor_at(o, to);
    const int c0 = o->first_chunk[t0], c1 = o->first_chunk[t1];
    if (o->kind == MI_OPT_LARS || want_norms) {
        if (mid_optim_norms(s, p, g, o->chunks_dev, c0, c1, o->part_dev)) return -1;
        if (mid_optim_trust(s, o->part_dev, o->first_chunk_dev, o->is_weight_dev, t0, t1, o->trust_coef, wd, o->sq_dev, o->trust_dev)) return -1;
    }
    return mid_optim_update(s, o->kind, p, g, b, o->chunks_dev, c0, c1, o->is_weight_dev, o->trust_dev, lr, wd, wd_norm, o->momentum, nan_flag);
}

/* momentum SGD or LARS instead of Adam; before the first update_parameters (later, the momentum arena would hold Adam moments) */
int mi_trainer_set_optimizer(Train_ResNet *t, int kind, float momentum, float trust_coef) {
    MiCtx *c = ctx_of(t);
    if (c->n_updates > 0) {
        mi_record_host_error("mi_trainer_set_optimizer", "the optimizer is chosen before the first update_parameters");
        return -1;
    }
    if (kind != MI_OPT_ADAM && kind != MI_OPT_SGD && kind != MI_OPT_LARS) {
        mi_record_host_error("mi_trainer_set_optimizer", "unknown optimizer kind");
        return -1;
    }
    const Params *p = t->model->params;
    const int n = p->n_locations;
    int *isw = (int *)malloc(sizeof(int) * (size_t)n);
    /* locations[] holds (weight, gamma, beta) triples -- the stem, every convolution of every block -- then the FC weight */
    for (int i = 0; i < n; i++) isw[i] = i % 3 == 0;
    MiOptim o;
    const int rc = mi_optim_init(&o, kind, momentum, trust_coef, c->loc_off, p->sizes, isw, n);
    free(isw);
    if (rc) return -1;
    mi_optim_free(&c->optim);
    c->optim = o;
    c->wd_norm_set = 0; /* the second decay group is a setting of the SGD it was made under */
    return 0;
}
int mi_trainer_get_optimizer(const Train_ResNet *t) { return ((const MiCtx *)t->backend_ctx)->optim.kind; }
int mi_trainer_set_norm_weight_decay(Train_ResNet *t, float wd_norm) {
    MiCtx *c = ctx_of(t);
    const char *who = "mi_trainer_set_norm_weight_decay";
    if (c->optim.kind != MI_OPT_SGD) { mi_record_host_error(who, "MI_OPT_SGD only (Adam keeps the reference's rule, LARS never decays gamma / beta)"); return -1; }
    if (!(wd_norm >= 0.f) || isinf(wd_norm)) { mi_record_host_error(who, "wd_norm is finite and >= 0"); return -1; }
    c->wd_norm = wd_norm; c->wd_norm_set = 1;
    return 0;
}

/* Gradient clipping (resnet_mi.h): update_parameters scales the gradient the optimizer is about to see so that its global L2 norm is at
 * most max_norm -- three launches on the compute stream, the coefficient stays on the device */
int mi_trainer_set_clip_grad_norm(Train_ResNet *t, float max_norm) {
    MiCtx *c = ctx_of(t);
    const char *who = "mi_trainer_set_clip_grad_norm";
    if (!(max_norm >= 0.f) || isinf(max_norm)) { mi_record_host_error(who, "max_norm is finite and >= 0 (0: off)"); return -1; }
    if (c->acc_pending > 0) { mi_record_host_error(who, "a window is open: micro-batches are pending"); return -1; }
    if (c->acc_in_step) { mi_record_host_error(who, "not between forward_pass and update_parameters"); return -1; }
    if (max_norm > 0.f && !c->clip.rec_dev) { /* the first time: the chunk table of the gradient arena, the partials and the record */
        const Params *p = t->model->params;
        MiClip k;
        if (mi_clip_init(&k, who, c->loc_off, p->sizes, p->n_locations)) return -1;
        c->clip = k;
    }
    c->clip_max_norm = max_norm;
    return 0;
}
int mi_trainer_last_clip(Train_ResNet *t, MiClipRecord *out) {
    MiCtx *c = ctx_of(t);
    if (!c->clip.rec_dev || !out) { mi_record_host_error("mi_trainer_last_clip", !out ? "out is NULL" : "clipping was never on"); return -1; }
    mid_memcpy_d2h(out, c->clip.rec_dev, sizeof *out, G.compute);
    mid_stream_sync(G.compute);
    return mid_last_error()[0] ? -1 : 0;
}

/* resnet.cu:2910-2987.  No host synchronisation in here: the NaN / Inf flag is copied back asynchronously and read at the
 * next synchronisation point (forward_pass's pred copy), and with a communicator Adam runs bucket by bucket, each launch
 * waiting only for its own bucket's all-reduce -- the FC ... stage-3 updates run while the stem-side buckets are still on
 * the wire, and the host is free to queue the next load_new_batch / forward_pass behind them. */
void update_parameters(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    const Params *p = t->model->params;
    float *p_arena = mi_params_arena_base(p);
    const float cur_b1 = t->cur_mean_decay * t->base_mean_decay; /* decays advance BEFORE use (:2920-2921) */
    const float cur_b2 = t->cur_var_decay * t->base_var_decay;
    if (c->dump_every > 0 && t->cur_dump_id % c->dump_every == 0) {
        if (c->dp_pending) mid_stream_sync(G.comm); /* the dump reads the gradient arena: not while RCCL is reducing it */
        dump_trainer(t->cur_dump_id, t, t->dump_dir);
    }
    mid_event_record(c->ev_t[4], G.compute);
    c->acc_in_step = 0;
    if (c->acc_k > 1) {
        if (acc_collecting(c)) { /* behind backward, whose end joined the weight-gradient stream: the sum so far, and nothing else */
            ck(mid_grad_accumulate(G.compute, c->acc_arena, c->g_arena, c->arena_floats, c->acc_pending ? MID_ACC_ADD : MID_ACC_FIRST, 1.f),
               "gradient accumulation");
            c->acc_pending++;
            if (c->input_reset) { /* :2981-2982 */
                mid_memset(t->cur_batch->images, 0, (size_t)t->batch_size * t->cur_batch->image_size * sizeof(float), G.compute);
                mid_memset(t->cur_batch->correct_classes, 0, (size_t)t->batch_size * sizeof(int), G.compute);
            }
            mid_event_record(c->ev_t[5], G.compute);
            return;
        }
        /* the window's last micro-batch (data parallel: backwards_pass folded every bucket in front of its all-reduce) */
        if (!c->acc_folded) ck(mid_grad_accumulate(G.compute, c->acc_arena, c->g_arena, c->arena_floats, MID_ACC_FOLD, c->acc_scale), "gradient fold");
        c->acc_folded = 0; c->acc_pending = 0;
    }
    const float wd_norm = c->wd_norm_set ? c->wd_norm : t->weight_decay;
    if (c->clip_max_norm > 0.f) {
        /* the global norm is that of the whole all-reduced gradient: every bucket first, then one update over the arena (the overlap of
         * the early buckets' updates with the late buckets' all-reduce is the price) */
        if (c->dp_pending) {
            for (int b = 0; b < c->n_buckets; b++) mid_stream_wait_event(G.compute, c->bk_ev[b]);
            c->dp_pending = 0; c->n_buckets = 0;
        }
        ck(mi_clip_run(&c->clip, G.compute, c->g_arena, c->clip_max_norm), "gradient clipping");
    }
    if (c->dp_pending && c->n_buckets > 0) {
        for (int b = 0; b < c->n_buckets; b++) {
            mid_stream_wait_event(G.compute, c->bk_ev[b]);
            const size_t o = c->bk_from[b], n = c->bk_to[b] - c->bk_from[b];
            if (c->optim.kind != MI_OPT_ADAM)
                ck(mi_optim_step(&c->optim, G.compute, p_arena, c->g_arena, c->m_arena, o, o + n, t->learning_rate, t->weight_decay,
                                 wd_norm, c->nan_flag_dev, 0), c->optim.kind == MI_OPT_SGD ? "SGD" : "LARS");
            else
                ck(mid_adam(G.compute, p_arena + o, c->g_arena + o, c->m_arena + o, c->v_arena + o, n, t->learning_rate, t->weight_decay,
                            t->base_mean_decay, t->base_var_decay, cur_b1, cur_b2, t->eps, c->nan_flag_dev, 1, c->loc_off_dev, c->n_loc, o), "Adam");
        }
        c->dp_pending = 0; c->n_buckets = 0;
    } else {
        /* one launch over the whole arena (LARS: norm pass, trust ratios, update); it also clears the gradients (:2972-2978) */
        if (c->optim.kind != MI_OPT_ADAM)
            ck(mi_optim_step(&c->optim, G.compute, p_arena, c->g_arena, c->m_arena, 0, c->arena_floats, t->learning_rate, t->weight_decay,
                             wd_norm, c->nan_flag_dev, 0), c->optim.kind == MI_OPT_SGD ? "SGD" : "LARS");
        else ck(mid_adam(G.compute, p_arena, c->g_arena, c->m_arena, c->v_arena, c->arena_floats, t->learning_rate, t->weight_decay,
                    t->base_mean_decay, t->base_var_decay, cur_b1, cur_b2, t->eps, c->nan_flag_dev, 1, c->loc_off_dev, c->n_loc, 0), "Adam");
    }
    if (c->input_reset) { /* :2981-2982 */
        mid_memset(t->cur_batch->images, 0, (size_t)t->batch_size * t->cur_batch->image_size * sizeof(float), G.compute);
        mid_memset(t->cur_batch->correct_classes, 0, (size_t)t->batch_size * sizeof(int), G.compute);
    }
    c->n_updates++;
    /* weight averaging: behind the optimizer (data parallel: behind the last bucket's update), one launch per arena on this stream */
    if (c->ema_every > 0 && c->n_updates % c->ema_every == 0) {
        const float w = mi_ema_weight(c->ema_decay, c->ema_warmup, c->ema_updates);
        ck(mid_ema_update(G.compute, c->ema_arena, p_arena, c->arena_floats, w), "EMA (parameters)");
        ck(mid_ema_update(G.compute, c->ema_rs, c->rs_arena, 2 * (size_t)c->rs_channels, w), "EMA (running statistics)");
        c->ema_updates++;
    }
    mid_event_record(c->ev_t[5], G.compute);
    mid_memcpy_d2h(c->nan_flag_host, c->nan_flag_dev, sizeof(int), G.compute);
    mid_event_record(c->ev_nan, G.compute);
    c->nan_check_pending = 1;
    c->params_dirty = 1; /* the re-laid weight copies are stale until the next forward_pass */
    t->cur_mean_decay = cur_b1;
    t->cur_var_decay = cur_b2;
}
/* end of an epoch as the reference's main() does it (resnet.cu:3410-3421): loss_per_epoch = the epoch's SUMMED loss,
 * accuracy_per_epoch = fraction right, data source rewound to the first shard, cur_epoch advanced */
void mi_trainer_end_epoch(Train_ResNet *t, float epoch_loss, float epoch_n_wrong, float total_images_per_epoch) {
    if (t->cur_epoch >= 0 && t->cur_epoch < (t->n_epochs > 0 ? t->n_epochs : 1)) {
        t->loss_per_epoch[t->cur_epoch] = epoch_loss;
        t->accuracy_per_epoch[t->cur_epoch] = (total_images_per_epoch - epoch_n_wrong) / total_images_per_epoch;
    }
    t->cur_batch->cur_shard_id = -1;
    t->cur_batch->cur_batch_in_shard = -1;
    t->cur_epoch += 1;
}
/* check_errors on demand (resnet.cu:2879-2907): waits for the device and reads the flag of the last update */
int mi_trainer_check_errors(Train_ResNet *t) {
    MiCtx *c = ctx_of(t);
    mid_stream_sync(G.compute);
    const int bad = c->nan_check_pending && *c->nan_flag_host;
    poll_nan_flag(t);
    return bad;
}
/* the locations[] index the last NaN / Inf report named (-1: none); mi_trainer_set_nan_exit(t, 0) makes the report return through
 * mi_trainer_check_errors instead of exit(1) (tests) */
/* storage type of the stem convolution's own output and of that tensor's gradient (MI_DTYPE_*): bf16 in the bf16 mode when the stem runs
 * on the matrix cores, fp32 otherwise (fp32 mode; VALU stem; RESNET_MI_BF16_STEM_TENSORS=f32) */
int mi_trainer_stem_dtype(Train_ResNet *t) { const MiCtx *c = ctx_of(t); return c->dtype == MID_BF16 && c->stem_bf16 ? MID_BF16 : MID_F32; }

int mi_debug_trainer_routes(const Train_ResNet *t, int *out, int cap) {
    const MiCtx *c = (const MiCtx *)t->backend_ctx;
    int n = 0;
    for (; n < c->n_units; n++) {
        const MiLayer *L = &c->units[n].L;
        if (4 * n + 4 <= cap) { out[4 * n] = L->fwd; out[4 * n + 1] = L->dgrad; out[4 * n + 2] = L->wgrad; out[4 * n + 3] = L->fz; }
    }
    return n;
}
int mi_trainer_nan_location(const Train_ResNet *t) { return ((const MiCtx *)t->backend_ctx)->nan_location; }
void mi_trainer_set_nan_exit(Train_ResNet *t, int on) {
    MiCtx *c = ctx_of(t);
    c->nan_no_exit = !on;
    if (on) return;
    /* a run that goes on after a report starts from a clean flag */
    mid_memset(c->nan_flag_dev, 0, sizeof(int), G.compute);
    mid_stream_sync(G.compute);
    *c->nan_flag_host = 0;
}

/* ---------------------------------------------------------------------------------------------- */
static void free_activations_host(Activations *a) {
    if (!a) return;
    free(a->norm_init_conv);
    for (int i = 0; i < a->n_conv_blocks; i++) {
        Activation_ConvBlock *k = a->activation_conv_blocks[i];
        free(k->norm_post_reduced); free(k->norm_post_spatial); free(k->norm_post_expanded); free(k->norm_post_projection);
        free(k);
    }
    free(a->activation_conv_blocks);
    free(a);
}
void destroy_trainer(Train_ResNet *t) {
    if (!t) return;
    MiCtx *c = ctx_of(t);
    mid_device_sync();
    const Dims *d = t->model->dims;
    for (MiCtx **pp = &g_live; *pp; pp = &(*pp)->next_live) if (*pp == c) { *pp = c->next_live; break; }
    mid_event_destroy(c->ev_nan);
    if (c->comm) mid_rccl_comm_destroy(c->comm);
    if (c->sync_bn_comm) { mid_bn_set_sync(NULL, 1, NULL, 0, 0); mid_rccl_comm_destroy(c->sync_bn_comm); mid_free(c->sync_bn_tmp); }
    for (int i = 0; i < c->n_allocs; i++) mid_free(c->allocs[i]);
    free(c->allocs); free(c->alloc_bytes);
    for (int i = 0; i < MI_MAX_BUCKETS; i++) mid_event_destroy(c->bk_ev[i]);
    mid_free_host(t->forward_buffer->pred_cpu);
    mid_free_host(c->nan_flag_host);
    mid_event_destroy(c->ev_grads); mid_event_destroy(c->ev_reduced);
    free(c->wt_tab);
    mid_event_destroy(c->ev_bn_done); mid_event_destroy(c->ev_wgrad_done);
    for (int i = 0; i < MI_RING; i++) mid_event_destroy(c->ring_ev[i]);
    for (int i = 0; i < 6; i++) mid_event_destroy(c->ev_t[i]);
    free_activations_host(t->forward_buffer->activations);
    free_activations_host(t->backprop_buffer->activation_derivs);
    free_params_host(t->backprop_buffer->param_derivs, d);
    free_params_host(t->backprop_buffer->prev_means, d);
    free_params_host(t->backprop_buffer->prev_vars, d);
    free(t->forward_buffer); free(t->backprop_buffer);
    mid_free(mi_params_arena_base(t->model->params));
    free_params_host(t->model->params, d);
    mi_batch_ext_free(t->cur_batch);
    free(t->model->dims); free(t->model);
    free(t->loss_per_epoch); free(t->accuracy_per_epoch);
    mi_optim_free(&c->optim);
    mi_clip_free(&c->clip);
    mid_free(c->mix_labels_b);
    free(c->erase_last);
    free(c->ta_last); mid_free(c->ta_workspace);
    mid_free(c->rs_arena); mid_free(c->rs_tab_dev); mid_free(c->eval_row); mid_free(c->eval_rank); mid_free(c->eval_metrics);
    mid_free(c->ema_arena); mid_free(c->ema_rs);
    mid_free(c->acc_arena);
    ev8_free(c);
    if (c->ev8_copied) mid_event_destroy(c->ev8_copied);
    free(c->loc_off);
    free(c->dump_root); free(c->units); free(c->blk_unit); free(c);
    free(t);
}

/* ---------------------------------------------------------------------------------------------- */
int mi_dp_unique_id_bytes(void) { return mid_rccl_unique_id_bytes(); }
int mi_dp_get_unique_id(void *out, int bytes) { return mid_rccl_get_unique_id(out, bytes); }
int mi_dp_init(Train_ResNet *t, int rank, int world, const void *unique_id, int bytes) {
    MiCtx *c = ctx_of(t);
    if (world < 1 || rank < 0 || rank >= world) return -1;
    if (world == 1 && !unique_id) { c->world = 1; return 0; }
    /* world == 1 with an id builds a one-rank communicator: the whole bucket/stream/event path runs (self-test) */
    c->comm = mid_rccl_comm_init(rank, world, unique_id, bytes);
    if (!c->comm) return -1;
    c->rank = rank; c->world = world;
    return 0;
}
void mi_dp_set_bucket_bytes(Train_ResNet *t, size_t bytes) { ctx_of(t)->bucket_bytes = bytes; }
/* Cross-replica batch norm ("offer sync-BN as an option, default off" -- the reference has none): statistics and
 * the (dbeta, dgamma) sums of every BN layer are all-reduced over the replicas, through a communicator of its own (the
 * gradient buckets' collectives run concurrently on the comm stream).  unique_id: a SECOND id from mi_dp_get_unique_id,
 * broadcast like the first.  With it, DP-N equals one replica at batch N x 256 up to summation order. */
int mi_dp_enable_sync_bn(Train_ResNet *t, const void *unique_id, int bytes) {
    MiCtx *c = ctx_of(t);
    if (!unique_id) { c->sync_bn = 0; mid_bn_set_sync(NULL, 1, NULL, 0, 0); rs_build_table(t); return 0; }
    if (c->sync_bn_comm) { c->sync_bn = 1; rs_build_table(t); return 0; }
    c->sync_bn_comm = mid_rccl_comm_init(c->rank, c->world, unique_id, bytes);
    if (!c->sync_bn_comm) return -1;
    const size_t nf = MI_SYNC_BN_TMP_FLOATS;
    c->sync_bn_tmp = (float *)mid_malloc(nf * sizeof(float));
    mid_bn_set_sync(c->sync_bn_comm, c->world, c->sync_bn_tmp, nf, 1);
    c->sync_bn = 1;
    rs_build_table(t); /* the running variances' sample count now spans the replicas */
    return 0;
}
int mi_dp_world(const Train_ResNet *t) { return ((MiCtx *)t->backend_ctx)->world; }

/* host-only view of the bucket plan (no GPU touched): the cuts backwards_pass will make for this network */
int mi_debug_dp_plan(const Dims *d, size_t bucket_bytes, size_t *from, size_t *to, int max) { return mi_dp_plan_buckets(d, bucket_bytes, from, to, max); }
size_t mi_debug_arena_floats(const Dims *d) { size_t a; (void)count_locations(d, &a); return a; }
/* the buckets the last backwards_pass actually handed to RCCL (valid until update_parameters) */
int mi_debug_last_buckets(const Train_ResNet *t, size_t *from, size_t *to, int max) {
    const MiCtx *c = (const MiCtx *)t->backend_ctx;
    for (int i = 0; i < c->n_buckets && i < max; i++) { from[i] = c->bk_from[i]; to[i] = c->bk_to[i]; }
    return c->n_buckets;
}
