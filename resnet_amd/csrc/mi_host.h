/* mi_host.h -- internal host-side state shared by trainer.c / layer.c / loader.c / dump.c / ops.c (plain C). */
#ifndef MI_HOST_H
#define MI_HOST_H
#include "mi_device.h"
#include "resnet_mi.h"

struct MiRng { uint64_t seed; uint64_t counter; };

/* splitmix64 counter streams (synth.c) -- identical to tests/synth.py */
uint64_t mi_splitmix64_at(uint64_t seed, uint64_t i);
void mi_synth_uniform(float *out, size_t n, uint64_t seed, uint64_t offset, float lo, float hi);
void mi_synth_normal(float *out, size_t n, uint64_t seed, uint64_t offset, double var);
void mi_synth_labels(int *out, size_t n, uint64_t seed, uint64_t offset, int n_classes);

/* process-wide device state: one compute stream (everything the reference put on the default stream),
 * one communication stream (RCCL), one copy stream (H2D of the next batch) */
typedef struct {
    int ready;
    mid_stream compute, comm, copy, aux; /* aux: weight-gradient kernels, concurrent with the next layer's BN' */
} MiGlobal;
MiGlobal *mi_global(void);

/* data source attached to a Batch (the reference hard-codes its shard path, resnet.cu:1275) */
typedef struct BatchExt {
    Batch *batch;
    int source, layout, status;
    int rank, world; /* data parallel: this rank's slice of every global batch of a shard */
    char *shard_dir, *images_path, *labels_path;
    uint64_t seed_images, seed_labels;
    int n_classes, pool_batches, pool_next;
    float *pool_images; /* device, NCHW, pool_batches * n_images * image_size */
    int *pool_labels;   /* device */
    int *pool_labels_host;
    float *stage_dev;   /* device staging for NHWC -> NCHW */
    /* shard prefetch: batch t+1 is copied to the device on the copy stream while step t computes */
    int prefetch, have_next, next_shard_id, next_batch_in_shard;
    float *images_next, *stage_next, *pinned_next;
    int *labels_next, *labels_next_host;
    mid_event ev_next, ev_compute; /* copy done / compute stream's position when the target buffers were handed to the copy stream */
    uint64_t synth_step;
    /* MI_SRC_SHARDS_U8: the resident shard as bytes (whole dim_in^2 images) with its crop offsets, the augmentation choice, and per
     * buffer set (0: the blocking load / the batch in use, 1: the prefetched next batch; swapped with the images) a pinned and a
     * device staging buffer for the batch's bytes and for its plan */
    int u8_dim_in, aug_mode, aug_flip, u8_have_crops, have_plan, next_epoch;
    int rrc_antialias;           /* MI_AUG_RRC: the boxes go through the antialiased kernel (mi_batch_set_antialias) */
    uint64_t aug_seed;
    double rrc_scale[2], rrc_ratio[2]; /* MI_AUG_RRC: area share and aspect ratio, (lo, hi) each */
    uint8_t *u8_shard;           /* host, shard_n_images * dim_in^2 * 3 */
    int *u8_crops;               /* host, [shard_n_images][2] */
    uint8_t *u8_pinned[2], *u8_dev[2];
    int *plan_pinned[2], *plan_dev[2]; /* [n_images][3], MI_AUG_RRC: [n_images][5] (room for 5 always); plan_pinned[0] = the plan of the last load */
    struct BatchExt *next;
} BatchExt;
BatchExt *mi_batch_ext(Batch *b);
void mi_batch_ext_free(Batch *b);

/* the switches (environment) that decide what runs, read once per trainer by init_trainer and once per operator call: the planner is
 * handed them; the .hip files keep only tuning knobs of a kernel's own geometry (*_BM, *_TAIL, *_VW, ...) */
typedef struct {
    int cl_s1, cl_s1_dgrad;      /* RESNET_MI_BF16_CL_S1 / _CL_S1_DGRAD (0: stride-1 3x3 forward + wgrad / dgrad on the NCHW kernels) */
    int cl_s2, cl_dgrad2;        /* RESNET_MI_BF16_CL_S2 / _CL_DGRAD2 (0: stride-2 forward + wgrad / dgrad on the NCHW kernels) */
    int stem_mfma, bf16_stem;    /* RESNET_MI_STEM_MFMA / RESNET_MI_BF16_STEM (0: the stem on the VALU kernels) */
    int stem_tensors_f32;        /* RESNET_MI_BF16_STEM_TENSORS=f32: the bf16 stem's output and its gradient stay fp32 tensors */
    int bnfuse_bwd;              /* RESNET_MI_BF16_BNFUSE_BWD (0: no BN' reduction in any dgrad, either storage type) */
    int bnfuse_bwd_f32;          /* RESNET_MI_F32_BNFUSE_BWD: fp32 site mask (see mi_layer_plan) */
    int overlap, overlap_given;  /* RESNET_MI_OVERLAP, and whether it was set at all */
    int bnfuse;                  /* RESNET_MI_BNFUSE (0: fp32 forward BN statistics by a pass of their own) */
    int prelayout;               /* RESNET_MI_PRELAYOUT (0: each fp32 convolution re-lays its own weights) */
    int igemm;                   /* RESNET_MI_IGEMM: which fp32 convolutions run on the matrix cores (0 none, 1 few, 2 all that tile; layer.c) */
    int pw_wgrad;                /* RESNET_MI_BF16_PW_WGRAD (0: every bf16 NCHW weight gradient on bgemm_kernel) */
} MiOptions;

/* One convolution of the network and how it runs (layer.c), decided once per build of the buffers: the kernel routes (MI_FWD_* /
 * MI_DG_* / MI_WG_*, resnet_mi.h) and the kernel of each (MI_K_*) follow from shape, storage type, store policy and options, and the
 * buffers the layer owns and their sizes follow from the kernels.  The trainer plans its table with the planner's own choices; an operator (ops.c) forces its routes. */
enum { MI_PLANNED = -1, MI_NOT_RUN = -2 }; /* a forced route: the planner's choice / the operation is not run and needs nothing */
typedef struct {
    const float *w;
    int C, H, K, k, stride;
    int N, dtype, out_dt;        /* batch, storage type of the activations, and of the convolution's own output (the stem's may stay fp32) */
    const mid_wt_entry *we;      /* the weights re-laid once per forward pass (relayout_weights), or NULL */
    int wre_fwd, wre_dgrad;      /* which re-laid forms the routes read from a weight table, */
    size_t wre_floats;           /* and the floats of one */
    int fwd, dgrad, wgrad;       /* MI_FWD_* / MI_DG_* / MI_WG_* */
    int kfwd, kdgrad, kwgrad;    /* MI_K_*: the kernel each runner launches */
    int fz;                      /* the dgrad is asked to do the reduction pass of the BN' its output feeds too (mi_layer_dgrad) */
    /* bf16, channel-last input planes (kernels_cl_bf16.hip) read by the forward and the weight gradient: one zero-padded plane
     * (stride 1) or four parity planes (stride 2); cl_by_bn (set by the trainer, which knows the producer): the producing BN apply
     * writes them (the reduction BN for the 3x3, the expansion BN of the block above for a stride-2 projection), else a re-layout
     * pass in front of the forward.  MI_FWD_PW: the dense channel-last input of the 1x1 kernel */
    void *cl; size_t cl_bytes; int cl_by_bn;
    void *dye; size_t dye_bytes; /* MI_DG_CL / MI_DG_CL2: the output gradient re-laid channel-last (mi_layer_dy_relayout), read by dgrad and wgrad */
    /* bf16 stride 2: NCHW parity planes of the input; par_valid: the last forward left them there (the weight gradient reuses them) */
    void *par; size_t par_bytes; int par_valid;
    /* stem on the matrix cores: the batch as zero-padded parity planes + wave partials and re-laid weights (kernels_stem_bf16.hip) */
    void *xp; size_t xp_bytes; float *scratch; size_t scratch_floats;
} MiLayer;
/* the workspaces every convolution of a table shares: sized for the largest need of its layers */
typedef struct {
    mid_workspace ws;
    float *bn_ws;
    mid_bn_parts bn_parts;       /* statistics partials a forward convolution leaves for its batch norm; the BN' sums of a fusing dgrad */
} MiLayerWs;
typedef struct { size_t wt, part, bn_parts; int maxc; } MiLayerNeed;
struct MiCtx;
void mi_layer_init(MiLayer *L, const float *w, int C, int H, int K, int k, int stride);
/* host only, allocates nothing: routes, fz and every size of L from (dtype, policy, options, N, shape, site = the layer's bit in the
 * BN'-fusion site masks, 0: not a site).  force: NULL, or per operation MI_PLANNED, MI_NOT_RUN or a route.  Returns 0, or -2 where a
 * route's *_supported test refuses the shape or the storage type; where a tensor is past a route's size limit ("Size
 * limits") mi_last_error names it */
int mi_layer_plan(MiLayer *L, int dtype, int policy, const MiOptions *o, int N, int site, const int force[3]);
/* the planned buffers at exactly their sizes (halos zeroed), tracked by the trainer c, or untracked (c == NULL: mi_layer_free) */
void mi_layer_alloc(struct MiCtx *c, MiLayer *L);
void mi_layer_free(MiLayer *L);
/* no weight table (operators): the forms the channel-last routes read, made here by a launch each; e backs L->we and is freed with L */
int mi_layer_own_weights(MiLayer *L, mid_wt_entry *e, mid_stream s);
void mi_layer_need(const MiLayer *L, MiLayerNeed *need); /* raises *need to what L's routes ask of the shared workspaces */
void mi_layer_ws_alloc(struct MiCtx *c, MiLayerWs *w, const MiLayerNeed *need);
void mi_layer_ws_free(MiLayerWs *w);
/* the runners: each returns its launcher's code.  parts: NULL, or &w->bn_parts for the statistics partials of the output */
int mi_layer_x_relayout(const MiLayer *L, mid_stream s, const void *x);   /* x into L->cl (mi_layer_fwd does it unless cl_by_bn) */
int mi_layer_fwd(MiLayer *L, MiLayerWs *w, mid_stream s, const void *x, void *y, mid_bn_parts *parts);
int mi_layer_bn_fwd(const MiLayer *L, MiLayerWs *w, mid_stream s, const mid_bn_parts *parts, const void *conv_out, const float *gamma,
                    const float *beta, const void *residual, float *means, float *vars, void *y, float *xhat_out, float *norm_out, float eps,
                    int relu, const MiLayer *cl_reader);
int mi_layer_bn_apply(const MiLayer *L, mid_stream s, const void *conv_out, const float *gamma, const float *beta, const void *residual,
                      const float *means, const float *vars, void *y, float eps, int relu, const MiLayer *cl_reader);
int mi_layer_dy_relayout(const MiLayer *L, mid_stream s, const void *dy); /* dy into L->dye, before the dgrad and the weight gradient */
const mid_bn_bwd_parts *mi_layer_fz_request(const MiLayer *L, const MiLayerWs *w, mid_bn_bwd_parts *r, const void *x, const void *mask,
                                            const float *means);
int mi_layer_dgrad(const MiLayer *L, MiLayerWs *w, mid_stream s, const void *dy, void *dx, const void *addend, const mid_bn_bwd_parts *req,
                   mid_bn_bwd_parts *fz);
int mi_layer_wgrad(const MiLayer *L, MiLayerWs *w, mid_stream s, const void *x, const void *dy, float *dw);
int mi_bn_bwd_unit(MiLayerWs *w, mid_stream s, mid_bn_bwd_parts *fz, const void *x, int x_dt, const float *gamma, const float *beta,
                   const float *means, const float *vars, const void *dy, const void *mask_src, int mask_mode, void *gated_out, int a_dt,
                   void *dx, float *dgamma, float *dbeta, int N, int C, int P, float eps);
void mi_read_options(MiOptions *o); /* the process's switches (trainer.c) */
/* the kernel an MI_*_F32 route runs operation op (0 fwd, 1 dgrad, 2 wgrad) of a shape on: the planner's rule, for the plan queries too */
int mi_layer_f32_kernel(const MiOptions *o, int op, int N, int C, int H, int K, int k, int stride);

/* One convolution + batch norm unit of the trainer's network, and everything about it that is fixed until the buffers are rebuilt
 * (trainer.c, build_units).  Forward tensors, parameters and parameter gradients only: nothing here points into the derivative tree,
 * whose tensors overlap mode 2 re-points from the ring on every backward pass */
enum { MI_U_STEM, MI_U_RED, MI_U_SPA, MI_U_EXP, MI_U_PROJ };
typedef struct MiUnit {
    MiLayer L;
    int block, role;             /* block -1: the stem */
    int site;                    /* the layer's bit in the BN'-fusion site masks (mi_layer_plan; 0: not a site) */
    int rs_off;                  /* where its channels start in the running-statistics arena */
    const BatchNorm *bn;
    BatchNorm *dbn;              /* (gamma, beta) gradients */
    Cache_BatchNorm *cache;      /* batch statistics of the last forward_pass (FULL: x-hat and BN output too) */
    float *dw;                   /* weight gradient */
    const float *in;             /* NULL: the pass's images (stem) */
    float *conv_out, *act_out;   /* the convolution's output; BN (+ReLU | +residual+ReLU) of it */
    const float *residual;
    int relu;
    struct MiUnit *cl_reader;    /* the unit whose channel-last input planes this unit's BN apply writes (reduction -> spatial,
                                  * expansion -> the next block's projection), or NULL */
    const float *add; float *sum; /* FULL, expansion: the residual is added by a pass of its own, which keeps the pre-ReLU sum */
    float *out;                  /* what the units behind read: act_out, or that pass's output */
} MiUnit;

/* momentum SGD / LARS over a parameter-shaped arena (kernels_optim.hip): the chunk table and the per-chunk / per-tensor scratch,
 * built once per arena geometry */
typedef struct {
    int kind;                    /* MI_OPT_ADAM (nothing built) | MI_OPT_SGD | MI_OPT_LARS */
    float momentum, trust_coef;
    int n_tensors, n_chunks;
    size_t *off;                 /* host: n_tensors + 1 float offsets (tensor starts, then the arena's end) */
    int *first_chunk;            /* host: n_tensors + 1 */
    mid_chunk *chunks_dev;
    int *first_chunk_dev, *is_weight_dev;
    double *part_dev;            /* 2 per chunk: (sum w^2, sum g^2) */
    double *sq_dev;              /* 2 per tensor: the squared norms of the last LARS pass */
    float *trust_dev;            /* 1 per tensor */
} MiOptim;
/* off: n + 1 float offsets (multiples of 4), sizes: n tensor lengths (<= the offset gap), is_weight: n flags (1: LARS trust ratio
 * and weight decay; 0: BN gamma / beta).  Returns 0, or -1 with mi_last_error set. */
int mi_optim_init(MiOptim *o, int kind, float momentum, float trust_coef, const size_t *off, const int *sizes, const int *is_weight, int n);
void mi_optim_free(MiOptim *o);
/* one update of the tensors whose start lies in [from, to) (floats into the arena), stream-ordered; want_norms: SGD too runs the
 * norm pass (sq_dev filled) */
int mi_optim_step(const MiOptim *o, mid_stream s, float *p, float *g, float *b, size_t from, size_t to, float lr, float wd, float wd_norm,
                  int *nan_flag, int want_norms);
/* gradient clipping by the global L2 norm over a parameter-shaped arena (kernels_optim.hip): a chunk table of its own -- cut as
 * MiOptim's is, whatever the optimizer -- one double partial per chunk and the record, all in device memory */
typedef struct {
    int n_chunks;
    mid_chunk *chunks_dev;
    double *part_dev;
    mid_clip_record *rec_dev;    /* zeroed when built: the counters run from there */
    size_t bytes;                /* of the three allocations */
} MiClip;
/* off / sizes / n as mi_optim_init.  Returns 0, or -1 with mi_last_error set (bad offsets: before any device work) */
int mi_clip_init(MiClip *k, const char *who, const size_t *off, const int *sizes, int n);
void mi_clip_free(MiClip *k);
/* the three launches on s: norm, coefficient, scale */
int mi_clip_run(const MiClip *k, mid_stream s, float *g, float max_norm);

typedef struct MiCtx {
    MiLayerWs lw;
    /* weights re-laid for the implicit-GEMM kernel once per forward pass (one launch): host table (MiLayer.we points into it),
     * device copies for the kernel */
    mid_wt_entry *wt_tab;
    int wt_n, wt_tiles;
    mid_wt_entry *wt_tab_dev;
    int *wt_tile_entry_dev;
    MiOptions opt;
    /* the network, written down once per build of the buffers (build_units; drop_buffers empties it) and read by every pass: the
     * units in the order of the BN gammas in Params.locations -- the stem, then per block reduction, spatial, expansion and the
     * projection where there is one.  That order is the running-statistics arena's, mi_debug_trainer_routes' and the weight
     * table's.  blk_unit[i]: block i's reduction unit (unit_of) */
    MiUnit *units;
    int n_units, *blk_unit;
    int *nan_flag_dev, *nan_flag_host;
    int nan_check_pending;       /* update_parameters queued a copy of the flag; read it at the next host sync point */
    mid_event ev_nan;            /* recorded behind that copy */
    size_t *loc_off_dev; int n_loc; /* arena offsets of locations[] (+ the arena's end) for the Adam kernel's report */
    size_t *loc_off;             /* the same offsets on the host */
    int nan_location, nan_no_exit;  /* last reported locations[] index (-1 none); test hook: report without exit(1) */
    struct MiCtx *next_live;     /* registry of live contexts (communicator teardown on a fatal error) */
    int full_store, dump_every, input_reset;
    int dtype;                   /* MID_F32 | MID_BF16: storage type of activations and activation gradients */
    int policy;                  /* MI_STORE_FAST | MI_STORE_RECOMPUTE_BN | MI_STORE_FULL */
    int n_persist;               /* allocs[0 .. n_persist) survive a rebuild of the activation buffers */
    size_t act_bytes, dev_bytes; /* forward activations kept for backward / every tracked allocation */
    size_t *alloc_bytes;
    float *rc_buf[2];            /* RECOMPUTE_BN: scratch for the BN(+ReLU) tensors (forward: consumed at once; backward: re-derived) */
    int stem_bf16;               /* bf16 mode: the stem convolution's output and its gradient are bf16 tensors too (RESNET_MI_BF16_STEM_TENSORS=f32: fp32 as in round 2) */
    float *stem_dx;              /* bf16 mode: the stem convolution's output gradient stays fp32 */
    int counting_act;
    int overlap_set;             /* mi_trainer_set_overlap was called: keep the caller's mode */
    int params_dirty;            /* update_parameters ran since the last weight re-layout */
    MiOptim optim;               /* mi_trainer_set_optimizer: SGD / LARS instead of Adam (kind MI_OPT_ADAM: nothing built) */
    int n_updates;               /* update_parameters calls so far (the optimizer is chosen before the first) */
    /* mi_trainer_set_clip_grad_norm (0: off; the table is built at the first value > 0 and is not tracked in allocs[]) and
     * mi_trainer_set_norm_weight_decay (wd_norm_set 0: BN gamma / beta decay with weight_decay, as every tensor does) */
    float clip_max_norm;
    MiClip clip;
    float wd_norm; int wd_norm_set;
    /* mi_trainer_set_loss: the head of forward_pass (MI_LOSS_* flags; 0: the reference's soft-max, host loss, ce_deriv), and for
     * MI_LOSS_DEVICE the per-row outputs [batch] and the two records (last, total) the loss head writes */
    float loss_smoothing; int loss_topk, loss_flags;
    float *loss_row; int *loss_rank;
    mid_loss_metrics *loss_metrics;
    /* mi_trainer_set_mix (all 0 / NULL while off; labels_b is not tracked in allocs[]): the settings, the plan of the last
     * load_new_batch and the partners' labels [batch] the two-label head reads */
    int mix_on;
    double mix_alpha[2], mix_prob, mix_switch; /* [0] mixup, [1] CutMix */
    uint64_t mix_seed;
    MiMixPlan mix_last;
    int *mix_labels_b;
    /* mi_trainer_set_erase (all 0 / NULL while it was never on): the settings, and the boxes [batch][4] of the last load_new_batch in
     * host memory with the number of rows they hold */
    int erase_on, erase_rows;
    double erase_prob, erase_scale[2], erase_ratio[2];
    MiEraseFill erase_fill;
    uint64_t erase_seed;
    int *erase_last;
    /* mi_trainer_set_trivial_augment (all 0 / NULL while it was never on): the records [batch] of the last load_new_batch in host memory
     * with the number of rows they hold, and the device workspace of mi_op_trivial_augment for a whole batch */
    int ta_on, ta_rows;
    uint64_t ta_seed;
    MiTaRow *ta_last;
    void *ta_workspace;
    /* mi_trainer_track_running_stats (all NULL / 0 while off; none of it is tracked in allocs[]: it survives a rebuild of the
     * buffers): the arena [2][rs_channels] (running means, then running variances, units in the table's order at MiUnit.rs_off),
     * the per-unit table of bn_running_update_kernel on the device, the number of forward_pass updates so far; the eval pass's
     * own loss-head rows and records (last, total); acts_from_eval: the stored activations are an eval pass's, backwards_pass
     * refuses them */
    int rs_on, rs_channels;
    float rs_momentum, *rs_arena;
    mid_bn_run_entry *rs_tab_dev;
    int64_t rs_updates;
    float *eval_row; int *eval_rank;
    mid_loss_metrics *eval_metrics;
    int acts_from_eval;
    /* mi_trainer_set_ema (all NULL / 0 before the first call; not tracked in allocs[] either): the averaged copies of the parameter
     * arena [arena_floats] and of the running arena [2][rs_channels], the setting, the number of EMA updates so far; ema_eval: the
     * eval entry points score the averaged model (mi_trainer_eval_use_ema); ema_swapped: the arenas are exchanged right now, by
     * mi_trainer_eval_u8 around its batch loop -- the eval passes inside it do not exchange again */
    float *ema_arena, *ema_rs;
    double ema_decay;
    int ema_every, ema_warmup, ema_eval, ema_swapped;
    int64_t ema_updates;
    /* mi_trainer_set_accumulation (k 1, scale 1, arena NULL before the first k > 1; not tracked in allocs[] either): the sum of the
     * window's micro-batch gradient arenas [arena_floats], the setting, the micro-batches summed so far in this window; acc_in_step:
     * between forward_pass and update_parameters (the setter is refused); acc_folded: backwards_pass folded every data-parallel
     * bucket of this window's last micro-batch, update_parameters does not fold again */
    float *acc_arena, acc_scale;
    int acc_k, acc_pending, acc_in_step, acc_folded;
    /* mi_trainer_eval_u8: scratch of its own -- the decoded batch, and bytes / labels / plan on the device and pinned; the event
     * behind the last copies out of the pinned set */
    int ev8_dim_in;
    float *ev8_images; uint8_t *ev8_bytes_dev, *ev8_bytes_pinned;
    int *ev8_labels_dev, *ev8_labels_pinned, *ev8_plan_dev, *ev8_plan_pinned;
    mid_event ev8_copied;
    unsigned long host_epoch_seen; /* the process-wide host-write count (mi_copy_to_device) that re-layout was made at */
    char *dump_root;
    /* every device allocation of this trainer (freed by destroy_trainer) */
    void **allocs;
    int n_allocs, cap_allocs;
    /* contiguous parameter-shaped arenas with identical offsets: params, grads, m, v */
    size_t arena_floats;
    float *g_arena, *m_arena, *v_arena;
    /* data parallel */
    void *comm;
    int rank, world;
    size_t bucket_bytes;
    size_t dp_cursor; /* floats: gradients [dp_cursor, arena_floats) already handed to RCCL */
    mid_event ev_grads, ev_reduced;
    int dp_pending;
    /* buckets handed to RCCL during the last backwards_pass, in issue order (FC first): Adam of bucket b waits only for
     * bucket b's event, so the early buckets update while the late ones are still on the wire */
#define MI_MAX_BUCKETS 64
    size_t bk_from[MI_MAX_BUCKETS], bk_to[MI_MAX_BUCKETS];
    mid_event bk_ev[MI_MAX_BUCKETS];
    int n_buckets;
    int sync_bn;                 /* cross-replica batch-norm statistics (default off: the reference has none) */
    void *sync_bn_comm;          /* its own communicator: BN collectives run on the compute stream, the buckets' on the comm stream */
    float *sync_bn_tmp;
    /* weight-gradient overlap: wgrad(L) runs on the aux stream next to BN'(L-1); joined before the next dgrad */
    int overlap_wgrad, wgrad_pending; /* 0 serial, 1 wgrad next to the following BN' only, 2 free-running (ring of buffers) */
    mid_event ev_bn_done, ev_wgrad_done;
    /* mode 2: derivative tensors of the backward chain come from a ring; a slot remembers the aux-stream weight gradient
     * that still reads it, and the compute stream waits for exactly that kernel before the slot is written again */
#define MI_RING 10
    float *ring_buf[MI_RING];
    mid_event ring_ev[MI_RING];
    int ring_busy[MI_RING], ring_next;
    float *dpool[6]; /* the fixed U0,U1,A,B,C,D buffers of modes 0/1 */
    /* timing */
    mid_event ev_t[6];
    float last_ms[5];
} MiCtx;

#define MI_GUARD 256 /* bytes of slack in front of and behind every tensor the bf16 kernels read (see aalloc, mi_malloc) */
void *mi_ctx_alloc(MiCtx *c, size_t bytes);
void mi_params_mark_dirty(void);
/* buckets the data-parallel path cuts for a network (host-only arithmetic shared with backwards_pass): fills
 * from[] / to[] (float offsets into the gradient arena, issue order) and returns their number */
int mi_dp_plan_buckets(const Dims *d, size_t bucket_bytes, size_t *from, size_t *to, int max);
size_t mi_params_arena_floats(const Params *p);
float *mi_params_arena_base(const Params *p);
void mi_dp_reduce_ready(Train_ResNet *t, size_t from_float_offset, int force);
/* trainer.c, the last steps of load_new_batch while mixing is on: the plan of this load, the mix launch on Batch.images and the
 * partners' labels, on the compute stream */
void mi_trainer_mix_batch(Train_ResNet *t, Batch *b, int rank, int world);
/* trainer.c, in front of it while erasing is on: the boxes of this load and the erase launch on Batch.images, on the compute stream */
void mi_trainer_erase_batch(Train_ResNet *t, Batch *b, int rank, int world);
/* trainer.c, in front of that while TrivialAugmentWide is on: the records of this load and the launches on Batch.images, on the compute stream */
void mi_trainer_ta_batch(Train_ResNet *t, Batch *b, int rank, int world);
/* loader.c: e of mi_erase_plan (resnet_mi.h), the key of a step's rows and the noise seed the trainer passes */
uint64_t mi_erase_key(uint64_t seed, int epoch, int64_t step, int rank, int world);
/* trainer.c, for dump.c's restore: the whole averaged model from host arrays laid out as the two device arenas are (params: arena_floats
 * floats, padding words included; stats: 2 * rs_channels) and the counter; -1 before mi_trainer_set_ema */
int mi_trainer_ema_restore(Train_ResNet *t, const float *params_arena_host, const float *stats_host, int64_t updates);
/* trainer.c, for dump.c's restore: the accumulator from a host array laid out as the arena is (read only where pending > 0) and the
 * window's count; -1 without an accumulator or with a count outside [0, k) */
int mi_trainer_accum_restore(Train_ResNet *t, const float *arena_host, int pending);
void mi_trainer_poll_errors(Train_ResNet *t); /* load_new_batch: wait for and read the NaN / Inf flag of the last update */
void mi_record_host_error(const char *what, const char *detail); /* sets mi_last_error (runtime.hip) */
int mi_loss_args_ok(const char *who, float smoothing, int topk, int L); /* ops.c: the rules of mi_op_loss_head / mi_trainer_set_loss */

#endif
