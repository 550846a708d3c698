/*
 * resnet_mi.h -- C-ABI of libresnet_mi.so: the MI355X (gfx950) drop-in for the trainer
 * surface of als244/ResNet.
 *
 * The reference's headers declare only structs (resnet.h:4-215, resnet_cudnn.h:4-216); its
 * entry points are C++ functions defined in resnet.cu.  This header keeps the struct layouts
 * field-for-field in the reference's order (so code written against resnet.h keeps compiling and
 * every offset is unchanged) and declares the entry points with C linkage, each citing the
 * definition it replaces.  `bool` parameters became `int`; curandGenerator_t* became an opaque
 * seed handle (MiRng*); the cudnnHandle_t member of resnet_cudnn.h:213 is the opaque
 * `backend_ctx` slot (HIP streams, workspaces, RCCL communicator).
 *
 * Device memory layout: activations NCHW fp32 (north_star), weights KCRS as the reference
 * (resnet.cu:140), FC weights [in][out] (resnet.cu:1751-1759).  All device pointers below are
 * HIP device pointers owned by the trainer; nothing is freed before destroy_trainer().
 */
#ifndef RESNET_MI_H
#define RESNET_MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- reference struct layouts (resnet.h) ---------------- */
typedef struct { /* resnet.h:4-9 */
    char **labels;
    char **synsets;
    int *counts;
    int n_classes;
} Class_Metadata;

typedef struct { /* resnet.h:11-33 */
    int input;
    int init_kernel_dim;
    int init_conv_filters;
    int init_conv_stride;
    int init_maxpool_dim;
    int init_maxpool_stride;
    int n_conv_blocks;
    int *is_block_spatial_reduction; /* caller-owned */
    int final_depth;
    int output;
} Dims;

typedef struct { /* resnet.h:35-40 */
    int spatial_dim;
    int depth;
    float *gamma;
    float *beta;
} BatchNorm;

typedef struct { /* resnet.h:43-74 */
    int incoming_filters;
    int incoming_spatial_dim;
    int reduced_depth;
    int expanded_depth;
    int stride;
    float *depth_reduction;
    BatchNorm *norm_depth_reduction;
    float *spatial;
    BatchNorm *norm_spatial;
    float *depth_expansion;
    BatchNorm *norm_expansion;
    float *projection; /* NULL when incoming_filters == expanded_depth */
    BatchNorm *norm_projection;
} ConvBlock;

typedef struct { /* resnet.h:78-88 */
    float *init_conv_layer;
    BatchNorm *norm_init_conv;
    ConvBlock **conv_blocks;
    float *fully_connected;
    float **locations; /* every tensor, order of resnet.cu:838-943 */
    int *sizes;
    int n_locations; /* COUNTED (3 + 9n + 3*#projections + 1), not the reference's 16+9n (:819) */
} Params;

typedef struct { /* resnet.h:90-97 */
    int input_size;
    int feature_size;
    float *means;
    float *vars;
    float *normalized_temp; /* x-hat; NULL unless the trainer stores full activations */
    float *normalized;      /* BN output before ReLU; NULL unless full-store */
} Cache_BatchNorm;

typedef struct { /* resnet.h:99-133 */
    int incoming_filters;
    int incoming_spatial_dim;
    int reduced_depth;
    int expanded_depth;
    int stride;
    float *post_reduced;
    Cache_BatchNorm *norm_post_reduced;
    float *post_reduced_activated;
    float *post_spatial;
    Cache_BatchNorm *norm_post_spatial;
    float *post_spatial_activated;
    float *post_expanded;
    Cache_BatchNorm *norm_post_expanded;
    float *post_expanded_norm_vals;
    float *transformed_residual;
    Cache_BatchNorm *norm_post_projection;
    float *post_projection_norm_vals;
    float *output;           /* pre-ReLU sum; aliases output_activated unless full-store */
    float *output_activated;
} Activation_ConvBlock;

typedef struct { /* resnet.h:137-152 */
    float *init_conv_applied;
    Cache_BatchNorm *norm_init_conv;
    float *init_conv_activated;
    int *max_inds; /* flat NCHW argmax index */
    float *init_convblock_input;
    Activation_ConvBlock **activation_conv_blocks;
    int n_conv_blocks;
    float *final_conv_output_pooled;
    float *linear_output;
} Activations;

typedef struct { /* resnet.h:154-157 */
    Dims *dims;
    Params *params;
} ResNet;

typedef struct { /* resnet.h:160-166 */
    Activations *activations;
    float *pred;
    float *pred_cpu; /* valid when forward_pass returns */
} Forward_Buffer;

typedef struct { /* resnet.h:168-174 */
    float *output_layer_deriv;
    Params *param_derivs;
    Params *prev_means;
    Params *prev_vars;
    Activations *activation_derivs;
} Backprop_Buffer;

typedef struct { /* resnet.h:176-192 */
    int image_dim;
    int image_size;
    int n_images;
    int cur_shard_id;
    int cur_batch_in_shard;
    int shard_n_images;
    float *full_shard_images;
    int *full_shard_correct_classes;
    float *images_float_cpu; /* pinned */
    float *images;           /* device, NCHW */
    int *correct_classes_cpu; /* pinned; valid after load_new_batch */
    int *correct_classes;
} Batch;

typedef struct { /* resnet.h:195-215, with resnet_cudnn.h:213's handle slot */
    ResNet *model;
    Batch *cur_batch;
    Forward_Buffer *forward_buffer;
    Backprop_Buffer *backprop_buffer;
    float learning_rate;
    float weight_decay;
    float base_mean_decay;
    float base_var_decay;
    float cur_mean_decay;
    float cur_var_decay;
    float eps;
    int batch_size;
    int n_epochs;
    int cur_dump_id;
    int cur_epoch;
    float *loss_per_epoch;
    float *accuracy_per_epoch;
    int init_loaded;
    void *backend_ctx; /* resnet_cudnn.h:213 cudnnHandle_t -> opaque MiCtx* */
    const char *dump_dir;
} Train_ResNet;

typedef struct MiRng MiRng; /* stands in for curandGenerator_t (resnet.cu:3264-3267) */

/* ---------------- entry points the reference's main() calls ---------------- */
/* resnet.cu:666 */
Dims *init_dimensions(int input, int init_kernel_dim, int init_conv_filters, int init_conv_stride,
                      int init_maxpool_dim, int init_maxpool_stride, int n_conv_blocks,
                      int *is_block_spatial_reduction, int final_depth, int output);
/* curandCreateGenerator + curandSetPseudoRandomGeneratorSeed, resnet.cu:3266-3267 */
MiRng *mi_rng_create(uint64_t seed);
void mi_rng_destroy(MiRng *);
/* resnet.cu:951 (Glorot-normal var 2/(fan_in+fan_out), FC var 1e-4, gamma 1, beta 0) */
ResNet *init_resnet(Dims *dims, MiRng *gen);
/* resnet.cu:1196 */
Batch *init_general_batch(int n_images, int image_size, int image_dim, int shard_n_images);
/* resnet.cu:1157 */
Train_ResNet *init_trainer(ResNet *model, Batch *cur_batch, int batch_size, float learning_rate, float weight_decay,
                           float mean_decay, float var_decay, float eps, int n_epochs, const char *dump_dir);
/* resnet_cudnn.cu:1160 (same, with the handle argument; `handle` is ignored) */
Train_ResNet *init_trainer_cudnn_abi(ResNet *model, Batch *cur_batch, int batch_size, float learning_rate,
                                     float weight_decay, float mean_decay, float var_decay, float eps, int n_epochs,
                                     void *handle, const char *dump_dir);
/* resnet.cu:1363 */
Class_Metadata *populate_class_info(char *label_filename, char *synset_filename, char *class_size_filename,
                                    int n_classes);
/* resnet.cu:1235 */
void load_new_batch(Train_ResNet *trainer, Class_Metadata *class_metadata, Batch *batch_buffer);
/* resnet.cu:1526: fills forward_buffer->pred and pred_cpu (blocks until pred_cpu is valid) */
void forward_pass(Train_ResNet *trainer);
/* resnet.cu:1777: fills backprop_buffer->param_derivs */
void backwards_pass(Train_ResNet *trainer);
/* resnet.cu:2910: Adam, zero gradients + batch buffers, advance decays, dump every 1000 steps */
void update_parameters(Train_ResNet *trainer);
/* resnet.cu:2755 / 2778 / 2821 */
void dump_trainer(int dump_id, Train_ResNet *trainer, const char *special_dir);
void overwrite_trainer_hyperparams(Train_ResNet *trainer, int dump_id, const char *special_dir);
void overwrite_model_params(Train_ResNet *trainer, int dump_id, const char *special_dir);

/* ---------------- additions (new symbols; nothing above changes) ---------------- */
int mi_device_count(void);
int mi_set_device(int device);       /* call before any init_* ; default device 0 */
const char *mi_last_error(void);     /* "" when no HIP/RCCL error has been recorded */
void mi_device_synchronize(void);    /* cudaDeviceSynchronize of the reference main loop */
void destroy_trainer(Train_ResNet *trainer); /* frees trainer, model, batch and every device buffer */

/* data source selection for load_new_batch (the reference hard-codes /mnt/storage paths, :1275) */
enum { MI_SRC_SHARDS = 0, MI_SRC_BUFFER = 1, MI_SRC_SYNTHETIC = 2, MI_SRC_HOST = 3 };
enum { MI_LAYOUT_NHWC = 0, MI_LAYOUT_NCHW = 1 };
/* shards: <dir>/%03d.images + %03d.labels (build_training_shards.c:150-160 / resnet.cu:1275-1285) */
void mi_batch_source_shards(Batch *b, const char *shard_dir, int layout);
/* overlap the H2D copy of batch t+1 with step t (copy stream, pinned double buffer); shard source only */
void mi_batch_set_prefetch(Batch *b, int on);
/* one dumped batch: images.buffer / labels.buffer (resnet.cu:1301-1311) */
void mi_batch_source_buffer(Batch *b, const char *images_path, const char *labels_path, int layout);
/* seeded synthetic stream kept resident in HBM: images U(-124,152), labels uniform */
void mi_batch_source_synthetic(Batch *b, uint64_t seed_images, uint64_t seed_labels, int n_classes, int pool_batches);
/* caller fills images_float_cpu / correct_classes_cpu itself before each load_new_batch */
void mi_batch_source_host(Batch *b, int layout);
/* 0 = exit(1) on a missing shard/buffer file like fopen failure should (reference leaves it unchecked, :1276) */
int mi_batch_last_status(const Batch *b);

/* options (set after init_trainer, before the first forward_pass) */
void mi_trainer_set_full_store(Train_ResNet *t, int on); /* also keep x-hat / BN-out / pre-ReLU sums (dump parity) */
void mi_trainer_set_dump_root(Train_ResNet *t, const char *root); /* replaces /mnt/storage/.../training_dumps */
void mi_trainer_set_dump_every(Train_ResNet *t, int every);       /* reference: 1000 (:2947); 0 disables */
void mi_trainer_set_input_reset(Train_ResNet *t, int on);
/* weight-gradient scheduling in backwards_pass.  0: everything on one stream, in the reference's order.  1: each layer's
 * weight gradient runs on a second stream next to the following layer's BN backward only (default).  2: weight gradients
 * run free on a low-priority second stream; the derivative tensors they read come from a ring of buffers and are only
 * rewritten after the reader has finished.  Results are bit-identical in all three modes. */
void mi_trainer_set_overlap(Train_ResNet *t, int mode);
float mi_host_loss(Train_ResNet *t, int *n_wrong);                /* resnet.cu:3363-3383 on pred_cpu */

/* raw device access for tests / weight injection (model_params/%03d.buffer semantics, resnet.cu:2845-2874) */
void mi_copy_to_device(void *dst_dev, const void *src_host, size_t bytes);
void mi_copy_to_host(void *dst_host, const void *src_dev, size_t bytes);

/* data parallel (new work): one process per GPU, RCCL all-reduce SUM of the gradient arena */
int mi_dp_unique_id_bytes(void);
int mi_dp_get_unique_id(void *out, int bytes);                        /* rank 0 */
int mi_dp_init(Train_ResNet *t, int rank, int world, const void *unique_id, int bytes);
void mi_dp_set_bucket_bytes(Train_ResNet *t, size_t bytes);
int mi_dp_world(const Train_ResNet *t);
/* option, default off (the reference has no cross-replica BN): batch-norm statistics and the (dbeta, dgamma) sums
 * taken over ALL replicas -- two all-reduces of [C] floats per BN layer in forward, one of [2C] in backward, through a
 * communicator of its own.  unique_id: a second id from mi_dp_get_unique_id (rank 0), broadcast like the first; call after
 * mi_dp_init.  NULL turns it off again. */
int mi_dp_enable_sync_bn(Train_ResNet *t, const void *unique_id, int bytes);

/* per-phase device timing of the last step in ms: [0]=load [1]=forward [2]=backward [3]=update [4]=allreduce wait */
void mi_trainer_last_timings(Train_ResNet *t, float out_ms[5]);

/* optional per-kernel-family timing with HIP events on the launch stream (used by bench.py's roofline):
 * family 0 direct (VALU) conv fwd/dgrad, 1 direct (VALU) conv wgrad, 2 1x1 conv / FC on MFMA, 3 batch norm,
 * 5 3x3 conv on the MFMA implicit GEMM (fwd, dgrad, wgrad), 4 the input-side passes (uint8 decode, NHWC -> NCHW, mixup / CutMix).
 * flops/bytes are the ALGORITHMIC work of the timed launches. */
void mi_prof_enable(int on); /* 0 off, 1 all families, otherwise a bit mask of (1 << family) */
void mi_prof_reset(void);
void mi_prof_get(int family, long *launches, double *ms, double *flops, double *bytes);

/* ---------------- operator layer (prepareAndDo* of resnet.cu:1386-1509), device pointers, NCHW ----------------
 * Exposed so parity tests can drive every kernel through the C-ABI on its own. `stream` NULL = the library's
 * compute stream. All return 0 on success. */
typedef void *mi_stream_t;
void *mi_malloc(size_t bytes);
void mi_free(void *p);
int mi_op_conv_fwd(const float *x, const float *w_kcrs, float *y, int N, int C, int H, int K, int k, int stride);
int mi_op_conv_dgrad(const float *w_kcrs, const float *dy, float *dx, int N, int C, int H, int K, int k, int stride,
                     int to_add);
int mi_op_conv_wgrad(const float *x, const float *dy, float *dw_kcrs, int N, int C, int H, int K, int k, int stride);
int mi_op_bn_fwd(const float *x, const float *gamma, const float *beta, float *means, float *vars, float *y, int N,
                 int C, int H, float eps, int relu);
/* y = relu(BN(x) + residual) fused (addVec + doActivation, resnet.cu:1717-1723) */
int mi_op_bn_fwd_add_relu(const float *x, const float *gamma, const float *beta, const float *residual, float *means,
                          float *vars, float *y, int N, int C, int H, float eps);
/* mask_mode 0 none, 1 own ReLU recomputed from x (activationAndBatchNormDeriv to_activate_deriv),
 * 2 external: dy is gated by mask_src > 0 (doActivationDeriv fused in, resnet.cu:1934) */
int mi_op_bn_bwd(const float *x, const float *gamma, const float *beta, const float *means, const float *vars,
                 const float *dy, const float *mask_src, float *dx, float *dgamma, float *dbeta, int N, int C, int H,
                 float eps, int mask_mode);
/* mask_mode 2 that also writes gated_out = (mask_src > 0 ? dy : 0): what backwards_pass uses for identity blocks, where the
 * gated upstream gradient is needed again as the shortcut addend (doActivationDeriv, resnet.cu:1934, without its own pass) */
int mi_op_bn_bwd_gate(const float *x, const float *gamma, const float *beta, const float *means, const float *vars,
                      const float *dy, const float *mask_src, float *gated_out, float *dx, float *dgamma, float *dbeta, int N,
                      int C, int H, float eps);
int mi_op_maxpool_fwd(const float *x, float *y, int *max_inds, int N, int C, int H, int k, int stride);
int mi_op_maxpool_bwd(const int *max_inds, const float *dy, float *dx, int N, int C, int H, int k, int stride);
int mi_op_avgpool_fwd(const float *x, float *y, int N, int C, int H);
int mi_op_avgpool_bwd(const float *dy, float *dx, int N, int C, int H);
int mi_op_relu_deriv(const float *x, const float *up, float *out, size_t n);
/* out[m x n] = A[m x k] * B[k x n], row-major (matMul, resnet.cu:70-85) and the two transposed forms
 * (prepareAndDoMatMulLeftTranspose / RightTranspose, resnet.cu:1482-1509) */
int mi_op_matmul(const float *A, const float *B, float *out, int m, int k, int n);
int mi_op_matmul_lt(const float *A_kxm, const float *B, float *out, int m, int k, int n);
int mi_op_matmul_rt(const float *A, const float *B_nxk, float *out, int m, int k, int n);
int mi_op_softmax(const float *x, float *out, int N, int L);
int mi_op_ce_deriv(const float *pred, const int *labels, float *d, int N, int L);
int mi_op_adam(float *p, const float *g, float *m, float *v, size_t n, float lr, float wd, float b1, float b2,
               float cur_b1, float cur_b2, float eps, int *nan_flag_dev);
int mi_op_nhwc_to_nchw(const float *in, float *out, int N, int H, int W, int C);
/* device-side seeded fill (splitmix64 counter stream, uniform [lo,hi)) -- synthetic operands for micro-benchmarks */
/* test aids against kernels that read LDS they did not write (LDS is not cleared between dispatches; tests/test_gpu_lds.py).
 * mi_debug_lds_fill: device synchronise, then a kernel on a private stream whose workgroups each own the largest dynamic LDS a workgroup may
 * have (the device attribute: all of a CU's LDS, so a workgroup sits alone on its CU), 8 workgroups per CU, each writing `word` to all of
 * it; device synchronise.  mi_debug_poison_lds is mi_debug_lds_fill(0xFFFFFFFF): NaN as fp32 and as both bf16 halves, 255 as a byte.
 * mi_debug_lds_probe: the same geometry reading only: out[0] workgroups run, [1] distinct CUs they ran on (hardware id registers), [2] words
 * examined, [3] words != word.  mi_debug_lds_geometry: out[0] the LDS bytes each of those workgroups owns, [1] the device's CU count
 * (multiProcessorCount), [2] workgroups per launch.
 * mi_debug_lds_fill_mode(on, word): while on, EVERY kernel launch of the library (any thread, any stream) is followed by device synchronise,
 * fill, device synchronise, so each kernel of an operator or a training step finds `word` in all LDS it does not write itself; switching
 * on fills once and restarts the counter mi_debug_lds_fills (fills since then).  The mode serialises launches and changes no value.
 * RESNET_MI_LDS_FILL=<hex word>, read once per process, switches it on from the first launch.  Out of its reach: words a kernel reads and
 * discards, and races inside a workgroup (those read the kernel's own earlier data, not the fill). */
int mi_debug_lds_fill(uint32_t word);
int mi_debug_poison_lds(void);
int mi_debug_lds_probe(uint32_t word, size_t out[4]);
int mi_debug_lds_geometry(size_t out[3]);
int mi_debug_lds_fill_mode(int on, uint32_t word);
size_t mi_debug_lds_fills(void);
/* test aid: red-zone mode of the device allocator behind every allocation of the library (operator tensors and workspaces, trainer, loader,
 * optimizer).  zone_bytes 0 = off (the default); else a multiple of 4096 (-1 otherwise): an allocation of b bytes becomes zone | b | zone, the
 * whole of it filled with fill_byte (0xFF: NaN as fp32 and bf16, -1 as int; 0x00: the control) before the pointer is returned.  Both zones
 * are compared with the fill when the allocation is freed and, for every live padded allocation, in mi_debug_redzone_check, after a device
 * synchronise.  The check returns the number of damaged allocations seen since the mode was last switched on, freed ones included, and
 * mi_last_error describes the first: serial number, payload bytes, front / back zone, first..last damaged offset from the payload's start
 * (front, negative) or end (back, from 0) and the number of damaged bytes.  Allocations keep the setting they were made under; switching
 * while some are live is safe.  mi_debug_redzone_stats: allocations verified and zone bytes compared since the mode was last switched on, and
 * padded allocations live now (any pointer may be NULL).  No access leaves the process's own allocations. */
int mi_debug_redzone(size_t zone_bytes, int fill_byte);
int mi_debug_redzone_check(void);
void mi_debug_redzone_stats(size_t *allocs_checked, size_t *zone_bytes_checked, size_t *live);
/* The launch ring (RESNET_MI_TRACE=1: the last 96 kernel launches, what the abort dump prints).  Each name carries the parameters that
 * select the kernel's instantiation, e.g. "bgemm_kernel<fwd,k3,s1,bm128,vw8,swp,sbuf>".  mi_debug_trace_names writes the names oldest
 * first, one per line, into buf (as many as fit in cap bytes, zero-terminated) and returns how many the ring holds (0 with the trace
 * off); mi_debug_trace_clear empties the ring. */
int mi_debug_trace_names(char *buf, size_t cap);
void mi_debug_trace_clear(void);
/* host-only (no GPU needed): route and grid the launch planners choose for a convolution.  op 0 fwd, 1 dgrad, 2 wgrad.
 * out[0] 1 = MFMA implicit GEMM / 0 = other kernels, [1] rows per tile, [2] tiles, [3] tiles launched whole, [4] reduction
 * slices per tail tile, [5] k-steps per slice, [6] wgrad splits, [7] workgroups per class or split, [8] k-steps */
int mi_debug_conv_plan(int op, int N, int C, int H, int K, int k, int stride, int out[9]);
int mi_op_fill_uniform(float *out, size_t n, uint64_t seed, float lo, float hi);
/* host-only (no GPU needed): the plan a convolution operator launches with, from the same planner functions the launchers call.
 * dtype MI_DTYPE_F32 (route DEFAULT: the implicit GEMM of mi_op_conv_*) or MI_DTYPE_BF16 (DEFAULT: the NCHW kernels of mi_op_conv_*_bf16;
 * CL: the channel-last 3x3 kernels of mi_op_conv_{fwd,dgrad,wgrad}_bf16_cl; CL2: mi_op_conv_wgrad_bf16_cl2; PW: mi_op_conv1x1_fwd_bf16_cl
 * and the LDS-DMA 1x1 weight gradient).  op 0 fwd, 1 dgrad, 2 wgrad; fwd / dgrad without a fused BN' reduction.
 * The plan is the one of a launch with the workspace the mi_op_* operators give it: the partial-tile buffer of the fp32 sliced tail
 * round, and for a bf16 NCHW stride-2 input its parity planes.  A launch without them plans differently (fp32: every tile whole; bf16
 * stride 2: element-wise staging, no padded columns), and so does an fp32 dgrad that fuses the BN' reduction (every tile whole).
 * out[0] rows per tile, [1] columns per tile, [2] tiles (a stride-2 dgrad: per parity class or row parity), [3] first tile of the sliced
 * tail round (= tiles: none), [4] reduction slices per tail tile, [5] weight-gradient splits launched (1: fwd / dgrad), [6] 1 = the split
 * reduce runs grouped.  Returns 0, or -2 where the route refuses the shape (out all 0). */
enum { MI_ROUTE_DEFAULT = 0, MI_ROUTE_CL = 1, MI_ROUTE_CL2 = 2, MI_ROUTE_PW = 3 };
int mi_conv_plan(int dtype, int route, int op, int N, int C, int H, int K, int k, int stride, int out[7]);
/* host-only (no GPU needed): the kernel routes the trainer's planner gives one convolution of a network at batch N, under the process's
 * RESNET_MI_* switches -- the planner the trainer and the mi_op_* convolution operators themselves run through.  dtype MI_DTYPE_*, policy
 * MI_STORE_*; site = the layer's bit in the BN'-fusion site masks (1 expansion, 2 spatial, 4 the reduction above an identity block, 0 none).
 * out = (forward, dgrad, wgrad route, 1 where the dgrad also does the reduction pass of the batch-norm backward its output feeds).
 * Returns 0, or -2 (out all 0): unknown dtype, policy or site, or a shape the storage type's kernels do not take -- at a batch past a
 * kernel's size limit mi_last_error says "size limit: ..." (the mi_op_* convolutions refuse the same way, before any launch).  A route is
 * a family of kernels; which kernel of the family runs is planned with it (mi_layer_kernels).  The LDS-DMA 1x1 weight gradient is not a
 * route of its own: it is one of MI_WG_BF16's two kernels. */
enum { MI_FWD_F32, MI_FWD_BF16, MI_FWD_CL, MI_FWD_STEM_F32, MI_FWD_STEM_BF16, MI_FWD_PW /* mi_op_conv1x1_fwd_bf16_cl only */ };
enum { MI_DG_F32, MI_DG_BF16, MI_DG_CL, MI_DG_CL2 };
enum { MI_WG_F32, MI_WG_BF16, MI_WG_CL, MI_WG_CL2, MI_WG_STEM_F32, MI_WG_STEM_BF16 };
int mi_layer_routes(int dtype, int policy, int N, int C, int H, int K, int k, int stride, int site, int out[4]);
/* host-only: the kernel of each operation inside those routes, out = (forward, dgrad, wgrad), arguments and return value as
 * mi_layer_routes.  Each id stands for one launcher; beside it the name its convolution launch leaves in the launch ring
 * (mi_debug_trace_names; the name goes on with "<" and the instantiation's parameters).  MI_*_F32 asks, in this order: the implicit GEMM
 * where RESNET_MI_IGEMM allows it (0: nowhere; 1: 1x1 weight gradients and the 3x3 stride-2 layers with K >= 2C, C >= 256; 2, the
 * default: everywhere) and its shape-and-size gate passes, the plain GEMM for a 1x1, then the direct kernels (a weight gradient: the C
 * form where its gate passes).  MI_WG_BF16 is the LDS-DMA kernel for the 1x1 shapes it tiles unless RESNET_MI_BF16_PW_WGRAD=0. */
enum {
    MI_K_NONE,        /* the operation is not run */
    MI_K_IGEMM,       /* "igemm_kernel"      MI_*_F32: fp32 implicit GEMM on the matrix cores */
    MI_K_GEMM1X1,     /* "gemm_mfma_kernel"  MI_*_F32: a 1x1 as a plain MFMA GEMM */
    MI_K_DCONV,       /* "dconv_kernel"      MI_FWD_F32 / MI_DG_F32: direct convolution */
    MI_K_WGRADC,      /* "wgradC_kernel"     MI_WG_F32: direct weight gradient, C form */
    MI_K_WGRAD,       /* "wgrad_kernel"      MI_WG_F32: direct weight gradient */
    MI_K_BGEMM,       /* "bgemm_kernel"      MI_*_BF16: bf16 NCHW */
    MI_K_PW_WGRAD,    /* "pw_wgrad_kernel"   MI_WG_BF16: LDS-DMA 1x1 weight gradient */
    MI_K_CL_CONV,     /* "cl_conv_kernel"    MI_FWD_CL / MI_FWD_PW / MI_DG_CL */
    MI_K_CL_DGRAD2,   /* "cl_dgrad2_kernel"  MI_DG_CL2 */
    MI_K_CL_WGRAD,    /* "cl_wgrad_kernel"   MI_WG_CL */
    MI_K_CL_WGRAD2,   /* "cl_wgrad2_kernel"  MI_WG_CL2 */
    MI_K_ST32_FWD,    /* "st32_fwd_kernel"   MI_FWD_STEM_F32 */
    MI_K_ST32_WGRAD,  /* "st32_wgrad_kernel" MI_WG_STEM_F32 */
    MI_K_ST_FWD,      /* "st_fwd_kernel"     MI_FWD_STEM_BF16 */
    MI_K_ST_WGRAD     /* "st_wgrad_kernel"   MI_WG_STEM_BF16 */
};
int mi_layer_kernels(int dtype, int policy, int N, int C, int H, int K, int k, int stride, int site, int out[3]);


/* ---------------- bf16-activation path (BASELINE configs[4]) ----------------
 * Activations and activation gradients stored as bf16 in the same NCHW tensors (the `float *` fields of Activations then
 * point at bf16 data, half the bytes), all arithmetic in fp32, convolutions on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation; parameters, parameter gradients, Adam state, BN statistics, the stem convolution's own output, the pooled
 * features and the FC / soft-max head stay fp32.  Structure mirrored: resnet_cudnn_nchw.cu:1196-1211 (NCHW tensors,
 * TENSOR_OP_MATH_ALLOW_CONVERSION), storage policy of resnet_cudnn_lowmem.cu:2152-2170. */
enum { MI_DTYPE_F32 = 0, MI_DTYPE_BF16 = 1 };
/* call after init_trainer and before the first load_new_batch / forward_pass: rebuilds the activation buffers at the new
 * element size.  Returns 0, or -1 (mi_last_error says why: a layer shape the bf16 kernels do not tile, full-store on). */
int mi_trainer_set_dtype(Train_ResNet *t, int dtype);
int mi_trainer_get_dtype(const Train_ResNet *t);
/* what backward keeps from forward.  FAST (default): per convolution the raw output and the BN(+ReLU) output, per block the
 * post-ReLU output.  RECOMPUTE_BN: raw convolution outputs, BN statistics and block outputs only; the BN(+ReLU) tensors are
 * re-derived in backward (resnet_clean.cu:2714, 2753, 2812; resnet_cudnn_lowmem.cu:2303-2313) -- bit-identical gradients,
 * fewer stored bytes.  FULL: FAST plus x-hat / BN-out / pre-ReLU sums (= mi_trainer_set_full_store, fp32 only). */
enum { MI_STORE_FAST = 0, MI_STORE_RECOMPUTE_BN = 1, MI_STORE_FULL = 2 };
int mi_trainer_set_store_policy(Train_ResNet *t, int policy);
/* bytes of device memory the trainer holds for forward activations (kept for backward) / for everything */
size_t mi_trainer_activation_bytes(const Train_ResNet *t);
size_t mi_trainer_device_bytes(const Train_ResNet *t);
void mi_clear_error(void);
/* check_errors on demand (resnet.cu:2879-2907): update_parameters no longer blocks to read the NaN / Inf flag of its Adam
 * launch; it is read at the next forward_pass, or here (waits for the device; dumps id 99999999 and exits like the reference
 * when set).  Returns 0 when clean. */
int mi_trainer_check_errors(Train_ResNet *t);
/* the locations[] index the last NaN / Inf report named -- "ERROR: nan or inf found at location: %d" (resnet.cu:2896; the
 * reference walks locations[] from the last to the first, :2952, so the highest offending index is the one it prints); -1 = none.
 * mi_trainer_set_nan_exit(t, 0): a report no longer ends the process (the reference's exit(1), :2899) but comes back through
 * mi_trainer_check_errors / mi_trainer_nan_location -- for tests. */
int mi_trainer_stem_dtype(Train_ResNet *t); /* storage type of activations->init_conv_applied (the stem convolution's own output) and of its gradient: MI_DTYPE_BF16 in the bf16 mode with the matrix-core stem, else MI_DTYPE_F32 */
/* the four numbers of mi_layer_routes for every convolution of a live trainer's table: the stem, then per block the reduction, the
 * spatial convolution, the expansion and (where the block has one) the projection.  Fills out[4 * i ..] for the first cap / 4 of them and
 * returns their number */
int mi_debug_trainer_routes(const Train_ResNet *t, int *out, int cap);
int mi_trainer_nan_location(const Train_ResNet *t);
void mi_trainer_set_nan_exit(Train_ResNet *t, int on);
/* test aid: the device-side merge of cross-replica batch norm (mi_dp_enable_sync_bn) on R replicas held by ONE process -- the
 * kernels the trainer launches around its collectives, with the all-reduce replaced by a sum over the R supplied buffers.
 * Device pointers [R][C]: means / vars (per-replica in, merged out), dgamma / dbeta (per-replica sums in, gradient-arena values
 * out = sum / R), sums_out [R][2C] (the sums each replica's dx formula sees) or NULL.  Either pair may be NULL. */
int mi_debug_bn_merge(int R, int C, float *means, float *vars, float *dgamma, float *dbeta, float *sums_out);
/* The update rule of update_parameters.  MI_OPT_ADAM (default): the reference's Adam.  MI_OPT_SGD: torch.optim.SGD with momentum,
 * dampening 0, no Nesterov, weight decay on every tensor (mi_trainer_set_norm_weight_decay gives BN gamma / beta their own): d = g + wd w; b = mu b + d; w -= lr b.  MI_OPT_LARS (You et al. 2017, the
 * MLPerf ResNet-50 form): convolution and FC weights b = mu b + lr trust (g + wd w); w -= b with trust = tau |w| / (|g| + wd |w|)
 * (1 where |w| or |g| is 0), the norms per tensor before any update; BN gamma / beta b = mu b + lr g; w -= b.  lr, wd = the trainer's
 * learning_rate / weight_decay, read at every update (a schedule writes learning_rate between steps).  b = the prev_means arena
 * (starts at zero, dumped as means/); prev_vars is not touched.  Guards as Adam's: a NaN / Inf gradient element keeps its w and b
 * and stays in the arena, finite gradients are cleared; LARS leaves a whole tensor as it is when a norm is not finite; the NaN flag
 * names the highest offending locations[] index.  Call before the first update_parameters (later: -1, mi_last_error says why); the
 * choice is not dumped, a resumed run sets it again. */
enum { MI_OPT_ADAM = 0, MI_OPT_SGD = 1, MI_OPT_LARS = 2 };
int mi_trainer_set_optimizer(Train_ResNet *t, int kind, float momentum, float trust_coef);
int mi_trainer_get_optimizer(const Train_ResNet *t);

/* ---------------- the loss head on the device: label smoothing, loss and top-k totals without the host ----------------
 * The reference's head is soft-max, a blocking copy of pred to the host, -logf(p_c) and a top-1 count there (mi_host_loss), and
 * pred - onehot in backwards_pass.  loss_head_kernel (kernels_loss.hip) does all of it in one launch, one wave per row r of logits
 * x[0..L) with label c, smoothing eps and u = eps / (float)L:
 *   pred      p_j = expf(x_j - mx) / s, mx = max_j x_j, s = sum_j expf(x_j - mx): the operations and the reduction order of mi_op_softmax,
 *             the same bits
 *   dlogits   p_j - t_j with t_c = (1.f - eps) + u and t_j = u otherwise: label-smoothed cross entropy, a batch SUM (no 1/N,
 *             resnet.cu:1806-1811); eps = 0: the bits of mi_op_ce_deriv
 *   row_loss  logf(s) - (1.f - eps) z_c - u sum_j z_j with z = x - mx: the shifted log-sum-exp form, finite where -logf(p_c) overflows
 *             (p_c = 0 once x_c is ~104 below the maximum) -- the one difference from mi_host_loss
 *   row_rank  #{ j != c : p_j >= p_c } on the p values as written: ties count against the label, the rule of mi_host_loss
 *             (resnet.cu:3363-3383).  Top-1 is wrong <=> rank >= 1, top-k is wrong <=> rank >= k.  A NaN p_c compares false with
 *             everything and gives rank 0, as the host rule does: that identity is kept.
 * A label outside [0, L): no t_c term (dlogits = p - u, what mi_op_ce_deriv does), row_rank = L, row_loss = NaN, nothing outside the
 * row is read.  A second one-wave launch sums row_loss in double, rows lane-strided then six exchange steps -- a fixed order, no
 * floating-point atomics, the same bits for the same input -- and counts rank >= 1 and rank >= topk into two records in device memory:
 * last (overwritten) and total (added to). */
typedef struct { double loss_sum; int64_t rows, wrong_top1, wrong_topk, batches; } MiLossMetrics;
/* device pointers; pred, dlogits [N][L], row_loss, row_rank [N], last_dev, total_dev: each may be NULL and is then neither computed nor
 * stored.  Returns 0, or -1 with mi_last_error set: smoothing outside [0, 1), topk outside [1, L], N or L < 1. */
int mi_op_loss_head(const float *logits, const int *labels, float *pred, float *dlogits, float *row_loss, int *row_rank, int N, int L,
                    float smoothing, int topk, MiLossMetrics *last_dev, MiLossMetrics *total_dev);
/* The trainer's head.  flags MI_LOSS_HOST (default, with smoothing 0 and topk 1): the reference's path above, launch for launch.
 * MI_LOSS_DEVICE: forward_pass runs the loss head in place of the soft-max -- pred (softmax.buffer of a dump is unchanged),
 * output_layer_deriv and the totals -- and backwards_pass launches no cross-entropy derivative; pred is still copied to pred_cpu and
 * forward_pass still blocks, so mi_host_loss works as before.  MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY: no copy and no stream
 * synchronise in forward_pass (the NaN / Inf flag of the last update is waited for by its own event), pred_cpu is not written, and
 * mi_host_loss synchronises and returns (float)last.loss_sum and last.wrong_top1, so a reference-style main loop runs unchanged.
 * Both storage types (the logits are fp32 in the bf16 mode too).  May be called between steps, not between forward_pass and
 * backwards_pass.  Returns 0, or -1 with mi_last_error set: smoothing outside [0, 1) or > 0 without MI_LOSS_DEVICE, topk outside
 * [1, output], NO_PRED_COPY without DEVICE, unknown flag bits.  Like the optimizer the setting is not dumped: a resumed run sets it again.
 * mi_trainer_metrics waits for the compute stream and copies the records of the last forward_pass and the running totals since the
 * last reset (either pointer may be NULL; reset_total != 0 zeroes the total afterwards); both all zero under MI_LOSS_HOST.  Data
 * parallel: the records are this rank's; summing them over the ranks is the caller's. */
enum { MI_LOSS_HOST = 0, MI_LOSS_DEVICE = 1, MI_LOSS_NO_PRED_COPY = 2 };
int mi_trainer_set_loss(Train_ResNet *t, float smoothing, int topk, int flags);
int mi_trainer_metrics(Train_ResNet *t, MiLossMetrics *last, MiLossMetrics *total, int reset_total);

/* ---------------- evaluation: batch-norm running statistics, the eval pass, validation metrics ----------------
 * The reference normalises with the statistics of the batch it is given, always.  Everything here is off by default, and with
 * nothing enabled every launch, value and file is what it was.  Nothing is folded into the convolution weights: the eval pass runs
 * the convolutions of forward_pass and the apply half of its batch norm (mid_bn_apply_t) with other statistics.
 *
 * mi_trainer_track_running_stats(t, on, momentum): call after init_trainer (and after mi_trainer_set_dtype, if used) and before the
 * first forward_pass.  Allocates one device arena [2][channels] of floats -- every layer's running means first, then every layer's
 * running variances, the layers in the order their gamma tensors appear in Params.locations (the stem, then per block reduction,
 * spatial, expansion, and projection where the block has one) -- with means 0, variances 1 and an update counter of 0.  While on,
 * forward_pass ends its batch-norm work with ONE launch of bn_running_update_kernel (kernels_bn.hip) over all layers, one thread per
 * channel, on the compute stream behind the last BN (under sync-BN it sees the merged statistics):
 *   rm = (1 - m) rm + m mean,   rv = (1 - m) rv + m (var unbias)
 * torch.nn.BatchNorm2d's rule: var = the biased batch variance Cache_BatchNorm.vars holds, unbias = mi_bn_unbias(n), n = batch_size x
 * plane (x the world size under sync-BN).  The counter goes up by one per forward_pass.  on = 0 stops the updates and refuses the eval
 * pass; the values stay, and on = 1 again goes on from them.  Returns 0, or -1 with mi_last_error set: momentum outside (0, 1].
 * Data parallel without sync-BN: each rank keeps the running statistics of its own batches; they are not averaged.
 * mi_bn_unbias (host-only, no GPU needed): n / (n - 1) computed in double and rounded to float; 1 where n <= 1.
 * mi_op_bn_running_update: the kernel on its own.  Host arrays of n_layers device pointers means_dev[i], vars_dev[i] ([channels[i]]
 * floats each), the channel counts and the sample counts n; running_dev = [2][running_channels] floats in device memory, layer i at the
 * sum of the channel counts before it in both halves; words past the layers' sum belong to no layer and are not touched.  Returns 0,
 * or -1 with mi_last_error set (checked before any device call): momentum outside (0, 1], no layer, a NULL array or pointer, a
 * channel count or sample count < 1, more channels than running_channels. */
int mi_trainer_track_running_stats(Train_ResNet *t, int on, float momentum);
float mi_bn_unbias(int64_t n);
int mi_op_bn_running_update(const float *const *means_dev, const float *const *vars_dev, const int *channels, const int64_t *counts, int n_layers,
                            float *running_dev, int running_channels, float momentum);
/* channels: the sum of the BN layers' channel counts (26 560 for ResNet-50), 0 before tracking was ever on.  get / set: host arrays
 * of `channels` floats each, in the arena's order; they wait for the compute stream.  set refuses (-1, nothing written) a value that
 * is not finite or a negative variance; both return -1 where tracking was never on.  mi_trainer_running_updates: the counter. */
int mi_trainer_running_stats_channels(const Train_ResNet *t);
int mi_trainer_get_running_stats(Train_ResNet *t, float *means, float *vars);
int mi_trainer_set_running_stats(Train_ResNet *t, const float *means, const float *vars);
int64_t mi_trainer_running_updates(const Train_ResNet *t);
/* The eval pass.  images_dev: fp32 NCHW [batch_size][3][input][input], the layout of Batch.images (t->cur_batch->images is a valid
 * argument); labels_dev: [batch_size] ints, or NULL for no metrics (pred is then written by the soft-max kernel).  It re-lays the
 * weights and walks the layers of forward_pass through the same convolution calls -- the launches and the output bits of training --
 * and behind each convolution the BN apply kernel with that layer's slice of the running arena: same gamma, beta and eps, same fused
 * residual + ReLU, same channel-last second output.  Max-pool, average pool and FC as in training; then the loss head over the first
 * n_valid rows only, smoothing 0, no dlogits (output_layer_deriv is not touched), pred written for those rows, into the trainer's own
 * EVAL records (mi_trainer_eval_metrics), not those of mi_trainer_metrics.  All batch_size rows go through the network; without batch
 * statistics no row sees another, so the rows from n_valid on change nothing.  It writes no Cache_BatchNorm.means / vars, running
 * statistic, counter, parameter, gradient or optimizer state, copies nothing to the host and synchronises nothing.  It overwrites the
 * stored activations of the last forward_pass: a backwards_pass behind it, with no new forward_pass in between, records an error in
 * mi_last_error and launches nothing.  Returns 0, or -1 with mi_last_error set: tracking off, the FULL store policy, n_valid outside
 * [1, batch_size], topk outside [1, output].
 * mi_trainer_eval_metrics: mi_trainer_metrics on the eval records.
 * mi_trainer_eval_u8: a whole host array of n images of dim_in x dim_in x 3 bytes (B,G,R, as the uint8 shards hold them) with n labels
 * in ceil(n / batch_size) eval passes.  It zeroes the eval total; per batch it copies bytes, labels and the MI_AUG_CENTER plan of
 * mi_augment_plan through pinned staging, decodes with the decode kernel into an image tensor of its own (Batch.images is not used),
 * zero-fills the image rows from n_valid = min(batch_size, remaining) on and runs the eval pass; at the end it synchronises once and
 * returns the total in *out (rows == n).  cur_dump_id, the Batch and the shard position are not touched.  -1 as the eval pass, and for
 * n < 1 or dim_in below the network's input.
 * Checkpoints: while tracking is on dump_trainer also writes <dump>/bn_running.buffer -- the arena's 2 x channels floats, then the
 * counter as int64 -- and overwrite_model_params restores both where the file exists; with tracking off a dump is byte for byte what
 * it was. */
int mi_trainer_eval_forward(Train_ResNet *t, const float *images_dev, const int *labels_dev, int n_valid, int topk);
int mi_trainer_eval_metrics(Train_ResNet *t, MiLossMetrics *last, MiLossMetrics *total, int reset_total);
int mi_trainer_eval_u8(Train_ResNet *t, const uint8_t *images_host, const int *labels_host, int64_t n, int dim_in, int topk, MiLossMetrics *out);
/* ---------------- weight averaging: an exponential moving average (EMA) of the model, and evaluation with it ----------------
 * torchvision's --model-ema / timm's ModelEmaV2 on the device.  Off by default; while mi_trainer_set_ema was never called every launch,
 * value and dumped file is what it was.
 *
 * The update is torch.lerp(e, p, w) on float32, one element at a time (ema_update_kernel, kernels_optim.hip):
 *   w <  0.5f :  e' = fmaf(w, p - e, e)
 *   w >= 0.5f :  e' = fmaf(-(1.f - w), p - e, p)          (p - e and 1.f - w each rounded to float once)
 *   e' not finite (p or e is not, or p - e overflows): the element keeps its value; no flag is raised
 * These are torch.lerp's bits; the unfused e + w (p - e) rounds twice and differs.  Where p == e the value stays (for w < 0.5f a -0.f
 * becomes +0.f), and w == 1.f gives p's bits (but a p of -0.f below e becomes +0.f).
 * mi_ema_weight(decay, warmup, k): host only, no GPU needed, a pure function.  k = the number of EMA updates done before this one;
 * d_k = warmup ? min(decay, (1 + k) / (10 + k)) : decay in double (timm's warm-up), w = (float)(1.0 - d_k); decay in [0, 1).  torchvision's
 * correction for averaging every `steps` updates of a batch of world x batch over `epochs` epochs (adjust = world batch steps / epochs,
 * decay' = 1 - min(1, (1 - decay) adjust)) is the caller's: pass the corrected decay.
 * mi_op_ema_update / mi_op_exchange: the two kernels on their own, on device arrays of n floats; exchange swaps a and b as 32-bit words
 * (NaN payloads and -0 survive).  Both pointers 16-byte aligned: 16-byte accesses with an element-wise tail of n % 4; otherwise an
 * element-wise instantiation.  -1 with mi_last_error set and nothing launched: a NULL pointer or one that is not 4-byte aligned, w
 * outside [0, 1] or NaN, overlapping ranges (exchange), n == 0, n > 2^40.
 *
 * mi_trainer_set_ema(t, decay, every, warmup).  What is averaged: the whole parameter arena (its padding words are zero and stay zero)
 * and the whole running-statistics arena (torchvision's use_buffers=True), with the same w.  The first call allocates both copies, fills
 * them from the current parameters and running statistics on the device and zeroes the EMA update counter; later calls change the
 * setting only.  While every >= 1, update_parameters ends -- behind the optimizer, under data parallel behind the last bucket's update, on
 * the compute stream, with no host synchronisation, copy or new stream -- with the two EMA launches in the update that brings the
 * trainer's update count to a multiple of `every`; w = mi_ema_weight(decay, warmup, counter), then the counter goes up.  every == 0
 * switches the updates off and keeps values and counter; switching on again continues from them.  Data parallel: every rank averages the
 * same parameters; without sync-BN each rank averages its own running statistics.  Returns 0, or -1 with mi_last_error set and nothing
 * changed: running statistics were never tracked (mi_trainer_track_running_stats: an averaged model could not be evaluated), decay
 * outside [0, 1) or NaN, every < 0.  May be called between steps.  Like the optimizer and the loss setting it is not dumped.
 * mi_trainer_ema_reset: the snapshot again, counter 0.  mi_trainer_ema_updates: the counter (0 before mi_trainer_set_ema).
 * mi_trainer_ema_get_location / _set_location: tensor i of locations[] of the averaged model, Params.sizes[i] floats on the host;
 * mi_trainer_ema_get_running_stats / _set_running_stats: as mi_trainer_get_running_stats / _set_running_stats.  The setters refuse (-1,
 * nothing written) a value that is not finite and a negative variance; all return -1 before mi_trainer_set_ema or for an index outside
 * locations[].
 *
 * mi_trainer_eval_use_ema(t, on): while on, mi_trainer_eval_forward and mi_trainer_eval_u8 score the averaged model.  exchange_kernel swaps
 * the parameter arena with its averaged copy and the running arena with its averaged copy, in place on the compute stream; the eval
 * trunk runs (it re-lays the weights at its start); the same launches swap back.  mi_trainer_eval_u8 exchanges once around its whole
 * batch loop.  No host copy, no synchronisation; the re-laid weight copies are marked stale, so no later pass uses the averaged ones.
 * BETWEEN THE TWO EXCHANGES THE PARAMETER ARENA HOLDS THE AVERAGED MODEL: an asynchronous read of Params.locations or of the running
 * statistics on a stream of the caller's must be ordered behind the call.  -1 before mi_trainer_set_ema.
 *
 * Checkpoints: once mi_trainer_set_ema was called (every == 0 included) dump_trainer also writes <dump>/ema/%03d.buffer -- raw fp32 per
 * locations[] index, the format of model_params/ -- and <dump>/ema_state.buffer: the counter as int64, then the averaged running arena's
 * 2 x channels floats.  overwrite_model_params on a trainer with mi_trainer_set_ema called restores both where they all exist and fit;
 * otherwise the averaged model becomes a snapshot of the restored parameters and statistics with counter 0 and one note goes to stderr. */
float mi_ema_weight(double decay, int warmup, int64_t k);
int mi_op_ema_update(float *ema, const float *p, size_t n, float w);
int mi_op_exchange(float *a, float *b, size_t n);
void mi_debug_ema_geometry(size_t out[4]); /* [0] threads of a workgroup, floats of its turn [1] vector [2] element-wise, [3] the grid's cap */
int mi_trainer_set_ema(Train_ResNet *t, double decay, int every, int warmup);
int mi_trainer_ema_reset(Train_ResNet *t);
int64_t mi_trainer_ema_updates(const Train_ResNet *t);
int mi_trainer_eval_use_ema(Train_ResNet *t, int on);
int mi_trainer_ema_get_location(Train_ResNet *t, int i, float *host);
int mi_trainer_ema_set_location(Train_ResNet *t, int i, const float *host);
int mi_trainer_ema_get_running_stats(Train_ResNet *t, float *means, float *vars);
int mi_trainer_ema_set_running_stats(Train_ResNet *t, const float *means, const float *vars);
/* ---------------- gradient accumulation: k micro-batches per optimizer update ----------------
 * The large global batches LARS and mixup / CutMix are made for, on the GPUs one has.  Off by default (k = 1); while off every launch,
 * value and dumped file is what it was, and nothing is allocated before the first k > 1.
 *
 * The gradient is a batch SUM (dlogits carries no 1/N), so the sum of k micro-batch gradients is what a batch k times as large would
 * have handed the optimizer -- batch norm statistics apart, which stay per micro-batch as in every framework.  A backward pass
 * OVERWRITES the gradient arena, so the sum lives in an accumulator arena of its own (grad_accum_kernel, kernels_optim.hip):
 *   MI_ACC_FIRST  acc = g                   as 32-bit words: NaN payloads and -0 as they are
 *   MI_ACC_ADD    acc = acc (+) g
 *   MI_ACC_FOLD   g = (acc (+) g) (x) scale  acc is not written
 * fp32, every operation rounded on its own (no fused multiply-add).  Nothing is guarded: a value that is not finite propagates by IEEE
 * rules, and the optimizer's own guards see a folded gradient that is not finite as they see any other.
 *
 * mi_op_grad_accumulate: the kernel on its own, on device arrays of n floats; 16-byte accesses where both pointers are 16-byte aligned,
 * element-wise otherwise.  -1, mi_last_error set, nothing launched or written: a NULL pointer, a pointer that is not 4-byte aligned,
 * overlapping ranges, n == 0 or n > 2^40, an unknown mode, in MI_ACC_FOLD a scale that is NaN, infinite or <= 0.
 *
 * mi_trainer_set_accumulation(t, k, scale): the main loop stays the reference's -- load_new_batch / forward_pass / backwards_pass /
 * update_parameters once per micro-batch.  Calls 1 .. k - 1 of a window to update_parameters only collect: one launch on the compute
 * stream (FIRST, then ADD), no optimizer, no EMA, no NaN-flag copy, no decay advance, the re-laid weights stay valid.  Call k folds
 * (scale: 1 for the sum, 1.f / k for the mean over micro-batches) and then does everything update_parameters does today, once: the
 * optimizer on the folded gradient (the LARS trust ratio is taken on it), the decay advance, the EMA (its `every` counts applied
 * updates), the NaN flag.  No new host synchronisation.  Per micro-batch stay the BN batch statistics and the running-statistics
 * update, cur_dump_id and the periodic dump, input_reset, the mix plan's step and the loss records.  Data parallel: the collecting
 * passes cut no bucket and start no collective; on the last pass every bucket is folded on the comm stream in front of its all-reduce
 * (scale per rank, before the sum), behind the events the all-reduce waits for.
 * The first call with k > 1 allocates the accumulator (counted in mi_trainer_device_bytes).  -1, mi_last_error set, nothing changed:
 * k < 1, a scale that is NaN, infinite or <= 0, a call inside a window (pending > 0) or between forward_pass and update_parameters.
 * mi_trainer_accumulation: k and the micro-batches summed so far in this window.  Like the optimizer, the setting is not dumped.
 *
 * Checkpoints: inside a window (k > 1, pending > 0) dump_trainer also writes <dump>/grad_accum.buffer -- k and pending as int32, then the
 * accumulator's arena floats; any other dump is byte for byte what it was.  overwrite_model_params on a trainer with k > 1 restores the
 * accumulator and pending where the file exists, holds the same k and fits; otherwise pending = 0, with one note on stderr if a file
 * was there.  mi_debug_accum_arena: the accumulator on the device (NULL before the first k > 1), laid out as the gradient arena. */
enum { MI_ACC_FIRST = 0, MI_ACC_ADD = 1, MI_ACC_FOLD = 2 };
int mi_op_grad_accumulate(float *acc, float *g, size_t n, int mode, float scale);
void mi_debug_accum_geometry(size_t out[4]); /* as mi_debug_ema_geometry */
int mi_trainer_set_accumulation(Train_ResNet *t, int k, float scale);
int mi_trainer_accumulation(const Train_ResNet *t, int *k, int *pending);
float *mi_debug_accum_arena(const Train_ResNet *t);
/* ---------------- gradient clipping by the global L2 norm: torchvision's --clip-grad-norm on the device ----------------
 * Off by default (max_norm 0); while off every launch, value and dumped file is what it was, and nothing is allocated before the first
 * max_norm > 0.  While on, update_parameters runs three launches on the compute stream in front of the optimizer (kernels_optim.hip), over a
 * chunk table that covers every tensor of the gradient arena and none of its padding, whatever the optimizer:
 *   norm    sum g^2 per chunk of at most 8192 floats in double (a float's square is exact there)
 *   coef    the partials summed by one wave in a fixed order; norm = sqrt(sq), coef = min(1, max_norm / (norm + 1e-6)) in double, rounded to
 *           float once -- torch.nn.utils.clip_grad_norm_'s coefficient -- into a record in device memory; the host never sees it
 *   scale   g = g * coef, one fp32 product per element, in place; where coef == 1.f no gradient word is read or written
 * No atomics and no host synchronisation: the same gradient gives the same record and the same scaled bits.
 * THE NON-FINITE RULE: where sq is NaN or Inf (a gradient element is), coef = 1, nonfinite = 1 and the gradient is left as it is; the
 * optimizers' own guards and the NaN flag then report it exactly as without clipping.  This departs on purpose from
 * torch.nn.utils.clip_grad_norm_, which would multiply every gradient by NaN.
 * THE UNITS OF max_norm are those of the gradient the optimizer sees: a batch SUM (dlogits carries no 1/N), summed over the k micro-batches
 * of an accumulation window times its scale, summed over the ranks under data parallel.  A recipe written for mean gradients multiplies its
 * max_norm by the batch size, or folds with scale = 1 / (k batch).
 * Order in update_parameters: accumulation fold, clip, optimizer, EMA.  Under accumulation the collecting calls do not touch the record; call
 * k clips the folded gradient once.  LARS takes its per-tensor norms from the clipped gradient.  Data parallel: the norm is that of the
 * all-reduced gradient, so with clipping on update_parameters waits for every bucket's event, clips the whole arena and runs the optimizer
 * in one launch over it (the same bits as bucket by bucket) -- the overlap of the early buckets' updates with the late buckets' all-reduce
 * is lost while clipping is on; with it off the bucket loop is untouched.
 * mi_trainer_set_clip_grad_norm(t, max_norm): 0 turns it off; may be called between updates.  The first call with max_norm > 0 allocates the
 * chunk table, the partials and the record (counted in mi_trainer_device_bytes; the record's counters start at 0).  -1, mi_last_error set,
 * nothing changed: NaN, Inf or a negative value, a call inside an accumulation window (pending > 0) or between forward_pass and
 * update_parameters.  Like the optimizer, the setting is not dumped.
 * mi_trainer_last_clip: waits for the compute stream and copies the record of the last clipped update -- sq_norm and norm BEFORE the
 * scaling (what torch returns), coef, nonfinite, and the running counters updates (clip passes) and clipped (those with coef < 1).  -1
 * before the first max_norm > 0.
 * mi_op_clip_grad_norm: the three kernels on their own over tensors [offsets_host[i], offsets_host[i + 1]) of the device array g of n
 * floats (n_tensors + 1 offsets, multiples of 4 below 2^31, the last <= n: the rule of mi_op_momentum_update); *out (host, may be NULL): the
 * record, counters from 0.  -1, mi_last_error set, nothing launched: g NULL or not 16-byte aligned, n == 0, bad offsets, a max_norm that
 * is NaN, infinite or <= 0. */
typedef struct { double sq_norm, norm; float coef; int nonfinite; int64_t updates, clipped; } MiClipRecord;
int mi_trainer_set_clip_grad_norm(Train_ResNet *t, float max_norm);
int mi_trainer_last_clip(Train_ResNet *t, MiClipRecord *out);
int mi_op_clip_grad_norm(float *g, size_t n, const size_t *offsets_host, int n_tensors, float max_norm, MiClipRecord *out);
/* for tools/bench_clip.py: the mean time in ms of one launch of the norm (pass 0), coefficient (1) or scale (2) kernel over reps launches,
 * between HIP events on the compute stream; arguments as mi_op_clip_grad_norm, a scale pass multiplies g by coef reps + 3 times; < 0: refused */
double mi_debug_clip_pass_ms(int pass, float *g, size_t n, const size_t *offsets_host, int n_tensors, float max_norm, int reps);
/* torchvision's --norm-weight-decay for MI_OPT_SGD: the tensors that are no convolution or FC weight (BN gamma / beta) decay with wd_norm
 * in place of the trainer's weight_decay -- torch.optim.SGD with two parameter groups.  Read at every update; until it is called gamma and
 * beta decay with weight_decay, which gives the bits SGD always gave.  Call after mi_trainer_set_optimizer (which forgets it).  -1,
 * mi_last_error set, nothing changed: the optimizer is Adam (the reference's rule stays) or LARS (which never decays them), a value that
 * is NaN, infinite or negative.  Not dumped. */
int mi_trainer_set_norm_weight_decay(Train_ResNet *t, float wd_norm);
/* the SGD / LARS kernels on their own: p, g, b device arrays of n floats; tensor i starts at offsets_host[i] (n_tensors + 1 entries,
 * multiples of 4, the last <= n) and runs to the next offset; tensor_is_weight_host[i] 1: trust ratio and weight decay (LARS).
 * nan_flag_dev: device int or NULL.  sq_norms_out_host (optional, 2 n_tensors doubles): (|w|^2, |g|^2) per tensor before the update,
 * for SGD too.  Returns 0, or -1 (mi_last_error says why).  mi_op_momentum_update2: under MI_OPT_SGD the tensors with
 * tensor_is_weight_host[i] == 0 decay with wd_norm (finite, >= 0) in place of wd; mi_op_momentum_update is it with wd_norm = wd. */
int mi_op_momentum_update(int kind, float *p, float *g, float *b, size_t n, const size_t *offsets_host, int n_tensors,
                          const int *tensor_is_weight_host, float lr, float wd, float momentum, float trust_coef, int *nan_flag_dev,
                          double *sq_norms_out_host);
int mi_op_momentum_update2(int kind, float *p, float *g, float *b, size_t n, const size_t *offsets_host, int n_tensors,
                           const int *tensor_is_weight_host, float lr, float wd, float wd_norm, float momentum, float trust_coef,
                           int *nan_flag_dev, double *sq_norms_out_host);
/* the end-of-epoch bookkeeping of the reference's main() (resnet.cu:3410-3421) */
void mi_trainer_end_epoch(Train_ResNet *t, float epoch_loss, float epoch_n_wrong, float total_images_per_epoch);
/* host-only (no GPU needed): the gradient buckets the data-parallel path cuts for a network -- float offsets [from, to) into
 * the gradient arena in issue order (FC side first).  mi_debug_last_buckets: what the last backwards_pass really issued. */
int mi_debug_dp_plan(const Dims *d, size_t bucket_bytes, size_t *from, size_t *to, int max);
size_t mi_debug_arena_floats(const Dims *d);
int mi_debug_last_buckets(const Train_ResNet *t, size_t *from, size_t *to, int max);

/* the offline shard writer, build_training_shards.c:13-167 with its literal paths as arguments: reads the partition CSV
 * ("CCC,NNNN,RR,CC" per line) and <class_dir>/%08d.buffer (uint8, dim_in x dim_in x 3, B,G,R), crops dim_out x dim_out at the
 * per-image offsets, converts to R,G,B floats minus 103.94 / 116.78 / 123.68, writes <out_dir>/%03d.images (fp32, NCHW like the
 * reference, or NHWC) and %03d.labels (int32).  Returns the number of images written, < 0 on error. */
int mi_build_shard(const char *partition_csv, const char *class_dir, const char *out_dir, int shard_id, int image_dim_in,
                   int image_dim_out, int layout);
/* data parallel: this rank's slice of every global batch of a shard ("each rank reads its slice of the same
 * shard/batch"): global batch g of a shard = images [g*world*N, (g+1)*world*N), rank r takes [.. + r*N, .. + (r+1)*N) */
void mi_batch_set_rank_slice(Batch *b, int rank, int world);

/* ---------------- uint8 shards with on-device crop, flip and decode ----------------
 * The fp32 shards above hold one crop per image, made once offline.  A uint8 shard keeps the class files' bytes as they are -- whole
 * dim_in x dim_in images, a third of the bytes of the 224^2 fp32 crop -- and the crop (+ flip, B,G,R -> R,G,B planes, mean subtraction)
 * is made on the device at every load (kernels_input.hip), so a new crop can be drawn every epoch.
 *
 * mi_build_shard_u8: same partition CSV and class files as mi_build_shard; writes <out_dir>/%03d.images_u8 ([n][dim_in][dim_in][3]
 * bytes, every image whole and unchanged, B,G,R interleaved), %03d.labels (int32, as mi_build_shard) and %03d.crops (int32 [n][2]: the
 * CSV's row and column offsets).  Returns the number of images, or -1 (no CSV), -2 (no class file), -4 (short class file). */
int mi_build_shard_u8(const char *partition_csv, const char *class_dir, const char *out_dir, int shard_id, int image_dim_in);
/* The augmentation plan of n consecutive images, host-only and deterministic: out[i] = (row_off, col_off, flip) of the image with global
 * index g = first_global_index + i.  FIXED: the offsets of fixed_crops ([n][2], the shard's .crops), no flip -- the reference's
 * behaviour.  CENTER: both offsets (dim_in - dim_out) / 2, no flip.  RANDOM: with R = dim_in - dim_out, s = splitmix64_at(seed, epoch),
 * r = splitmix64_at(s, g) (the counter streams of synth.c): row_off = ((r & 0xFFFFF) (R + 1)) >> 20, col_off = (((r >> 20) & 0xFFFFF)
 * (R + 1)) >> 20, flip = flip ? r >> 63 : 0.  Returns 0, or -1 (unknown mode, dim_out > dim_in, FIXED without fixed_crops or with an
 * offset outside [0, R]; mi_last_error says which). */
enum { MI_AUG_FIXED = 0, MI_AUG_CENTER = 1, MI_AUG_RANDOM = 2 };
int mi_augment_plan(int mode, int flip, uint64_t seed, int epoch, int64_t first_global_index, int n, int dim_in, int dim_out,
                    const int *fixed_crops, int *out);
/* the decode kernel on its own: src_dev n whole images of bytes (16-byte aligned, else -1), plan_dev int [n][3] as mi_augment_plan
 * writes it, out_nchw fp32 [n][3][dim_out][dim_out]: out[n][d][h][w] = (float)((double)(float)byte - mean) of the byte
 * src[n][row_off + h][col_off + (flip ? dim_out - 1 - w : w)][2 - d], mean = 123.68 / 116.78 / 103.94 for byte position 0 / 1 / 2 --
 * the bits mi_build_shard writes.  Offsets outside [0, dim_in - dim_out] are clamped; nothing outside the n images is read. */
int mi_op_decode_u8(const uint8_t *src_dev, const int *plan_dev, float *out_nchw, int n, int dim_in, int dim_out);
/* load_new_batch from <shard_dir>/%03d.images_u8 + .labels (+ .crops): the shard stays in host RAM as bytes; every load builds the plan
 * of this rank's images (global index = cur_shard_id * shard_n_images + position in the shard, epoch = trainer->cur_epoch: the values
 * dump_trainer saves, so prefetch, rank slices and a resumed run see the same pixels), copies the batch's bytes, labels and plan
 * through pinned buffers and decodes into Batch.images (fp32 NCHW, image_dim = the crop's size) on the same stream -- the compute
 * stream, or the copy stream for the prefetched next batch.  Shard rotation, ragged tail, rank slices, status -1 on a missing file and
 * the cur_batch_in_shard / cur_dump_id bookkeeping are those of MI_SRC_SHARDS; FIXED without a .crops file is status -1 too.
 * Batch.images_float_cpu and Batch.full_shard_images are NOT filled by this source (there is no host fp32 image). */
enum { MI_SRC_SHARDS_U8 = 4 };
void mi_batch_source_shards_u8(Batch *b, const char *shard_dir, int image_dim_in);
/* mode MI_AUG_* (default FIXED), flip 0 / 1 (RANDOM only), seed; MI_SRC_SHARDS_U8 only (else -1, mi_last_error set).  Like the
 * optimizer, mode and seed are not dumped: a resumed run sets them again. */
int mi_batch_set_augment(Batch *b, int mode, int flip, uint64_t seed);
/* the plan of the last load, int [n_images][3]; returns n_images, or -1 (another source, nothing loaded yet, or MI_AUG_RRC, whose plan
 * is mi_batch_last_boxes') */
int mi_batch_last_plan(const Batch *b, int *out);

/* ---------------- random-resized crop (RRC) from the uint8 shards ----------------
 * The modes above cut a dim_out^2 window: every image is seen at one scale.  MI_AUG_RRC draws a box of random area and aspect ratio per
 * image and epoch (torchvision's RandomResizedCrop.get_params on a square image) and the resample kernel (kernels_input.hip) scales it
 * to dim_out^2 -- bilinear, + flip, planes and mean subtraction as the decode.
 *
 * mi_augment_plan_rrc: out[i] = (row0, col0, box_h, box_w, flip) of the image with global index g = first_global_index + i, host-only, a
 * pure function of (seed, epoch, g).  s = splitmix64_at(seed, epoch), k = splitmix64_at(s, g), d(j) = splitmix64_at(k, j),
 * U(x) = (x >> 11) 2^-53.  Try t = 0 .. 9: target = dim_in^2 (scale_lo + U(d(4t)) (scale_hi - scale_lo)), ratio = exp(log(ratio_lo) +
 * U(d(4t + 1)) (log(ratio_hi) - log(ratio_lo))), w = lrint(sqrt(target ratio)), h = lrint(sqrt(target / ratio)) (half to even); the first
 * try with 1 <= w, h <= dim_in is taken, row0 = ((d(4t + 2) >> 32) (dim_in - h + 1)) >> 32, col0 = ((d(4t + 3) >> 32) (dim_in - w + 1)) >> 32.
 * No try taken: ratio_lo > 1: w = dim_in, h = lrint(dim_in / ratio_lo); ratio_hi < 1: h = dim_in, w = lrint(dim_in ratio_hi); else the
 * whole image; h, w clamped to [1, dim_in], the box centred.  flip = flip ? d(40) >> 63 : 0.  Plain double arithmetic, every operation
 * rounded on its own.  Returns 0, or -1 (n < 0, dim_in < 1, scale_lo or ratio_lo not positive, scale_hi < scale_lo, ratio_hi < ratio_lo). */
enum { MI_AUG_RRC = 3 };
int mi_augment_plan_rrc(int flip, uint64_t seed, int epoch, int64_t first_global_index, int n, int dim_in, double scale_lo, double scale_hi,
                        double ratio_lo, double ratio_hi, int *out);
/* the resample kernel on its own: src_dev as mi_op_decode_u8 (16-byte aligned, else -1), boxes_dev int [n][5] as mi_augment_plan_rrc
 * writes it, out_nchw fp32 [n][3][dim_out][dim_out].  The box is clamped first (h, w into [1, dim_in], row0 into [0, dim_in - h], col0
 * into [0, dim_in - w]): nothing outside the n images is read.  With D = dim_out, output row oy reads source rows y0 and
 * y1 = min(y0 + 1, h - 1) of the box with weight wy / 256 on y1: num = clamp((2 oy + 1) h - D, 0, (h - 1) 2 D), fy = floor(256 num / (2 D)),
 * y0 = fy >> 8, wy = fy & 255; columns likewise with w on ox' = flip ? D - 1 - ox : ox.  For byte position p (B, G, R) of the four
 * neighbours b: top = b00 (256 - wx) + b01 wx, bot = b10 (256 - wx) + b11 wx, v = top (256 - wy) + bot wy (<= 255 * 65536, exact in int32
 * and fp32), out[n][2 - p][oy][ox] = (float)((double)v 2^-16 - mean[p]), mean = 123.68 / 116.78 / 103.94.  A box with h = w = dim_out has
 * wx = wy = 0 everywhere: the bits of mi_op_decode_u8 on the plan (row0, col0, flip).  The kernel stages source rows in LDS sized for a
 * box as large as the image: with R output rows per workgroup (16, fewer where needed) it holds ceil((R - 1) dim_in / D) + 2 rows of
 * 16 ceil((3 dim_in + 15) / 16) bytes + 4 (D + R, each rounded up to 4) bytes of tables in 64 KB.  Returns -2 where R = 1 does not fit. */
int mi_op_resample_u8(const uint8_t *src_dev, const int *boxes_dev, float *out_nchw, int n, int dim_in, int dim_out);
/* MI_SRC_SHARDS_U8 only (else -1, mi_last_error set; -1 too for bounds mi_augment_plan_rrc refuses): load_new_batch builds the box plan
 * at the same (epoch, global index) as the RANDOM mode and resamples on the same stream; rotation, ragged tail, rank slices, prefetch
 * and resume are unchanged.  A later mi_batch_set_augment switches back.  Like the other modes it is not dumped. */
int mi_batch_set_augment_rrc(Batch *b, int flip, uint64_t seed, double scale_lo, double scale_hi, double ratio_lo, double ratio_hi);
/* the boxes of the last load, int [n_images][5]; returns n_images, or -1 (another source or mode, or nothing loaded yet) */
int mi_batch_last_boxes(const Batch *b, int *out);

/* ---------------- antialiased resize: Pillow's bilinear bits for the random-resized crop and the validation resize ----------------
 * mi_op_resample_u8 reads two source pixels per axis whatever the scale: a box larger than the output is point-sampled.  Pillow's
 * Image.resize(size, BILINEAR) -- what torchvision's RandomResizedCrop and Resize run on PIL images -- widens the triangle filter by the
 * scale factor instead, in fixed-point arithmetic on bytes with a stated rounding; the kernel below reproduces it bit for bit on the box
 * cut out first: img.crop(box).resize((V, V), BILINEAR).  tests/aaref.py restates it and is compared with Pillow itself.
 *
 * One axis scales `in` source pixels (the box's) to V output pixels.  In double, every operation rounded on its own (no fused
 * multiply-add, host or device):  scale = in / V, fs = max(scale, 1.0), support = fs, ss = 1.0 / fs.  Output index o:
 *   center = (o + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in), the cast
 *   truncating toward zero;  taps j = 0 .. xmax - xmin - 1:  a = fabs((j + xmin - center + 0.5) ss), w_j = a < 1.0 ? 1.0 - a : 0.0,
 *   ww = sum of w_j in order of j, k_j = w_j / ww, K_j = (int)(0.5 + k_j 4194304.0) -- 22 fractional bits;
 *   pixel = clip((2097152 + sum_j byte[xmin + j] K_j) >> 22, 0, 255), exact in int32 (at most 16384 taps of weights that sum to 2^22 +- taps / 2).
 * Two dimensions: the horizontal pass first, its result ROUNDED TO BYTES, the vertical pass on those bytes.  Pillow skips a pass whose
 * in == V; its table is K = (2^22, 0), which hands every byte through unchanged, so the kernel does not branch.  The filter never reads
 * outside the box.  The written value is the decode's: out[n][2 - p][oy][ox] = (float)((double)(float)byte - mean[p]).
 *
 * mi_aa_coeffs: host-only, no GPU: xmin and K_0 .. K_{min(taps, cap) - 1} of output index o, returns the tap count xmax - xmin (-1:
 * in or V < 1, o outside [0, V)).  It is compiled from the text the kernel compiles (csrc/mi_aa.h).
 *
 * mi_op_resample_aa_u8: src_dev, boxes_dev and out_nchw as mi_op_resample_u8, the boxes clamped the same way.  Every box is scaled to
 * virt x virt; of that the window of rows [win_row, win_row + dim_out) x columns [win_col, win_col + dim_out) is written, output column ox
 * taking window column flip ? dim_out - 1 - ox : ox.  The RRC uses virt = dim_out and window (0, 0); a validation resize the whole image
 * as box, virt = the resize size and the centre window.  A box with h = w = virt = dim_out gives mi_op_decode_u8's bits; an upscale does
 * NOT give mi_op_resample_u8's (another convention).  A workgroup owns R window rows of one image (16, fewer where needed): it builds
 * the tap tables of its rows and of the window's columns from the box, stages the source rows and columns those need (16-byte loads
 * that stay inside the n images), filters them horizontally into bytes in LDS and vertically from there.  LDS, sized for a box as
 * large as the image, with ks = 2 max(ceil(dim_in / virt), 1) + 1 the most taps of an output index and S the most source rows of R
 * output rows (dim_in >= virt: ceil((R + 1) dim_in / virt) + 1, else ceil((R - 1) dim_in / virt) + 3; at most dim_in):
 * 4 (dim_out + R)(ks + 2) bytes of tables rounded up to 16, + S (16 ceil((3 dim_in + 15) / 16) + 3 dim_out rounded up to 4) in 64 KB.
 * Returns 0; -2 where R = 1 does not fit; -1 with mi_last_error set and nothing launched: n outside [1, 65535], dim_in, dim_out or
 * virt outside [1, 16384], src not 16-byte aligned, out or boxes not 4-byte aligned, a window that leaves [0, virt]. */
int mi_aa_coeffs(int in, int V, int o, int *xmin, int *K, int cap);
int mi_op_resample_aa_u8(const uint8_t *src_dev, const int *boxes_dev, float *out_nchw, int n, int dim_in, int dim_out, int virt, int win_row,
                         int win_col);
/* MI_SRC_SHARDS_U8 only (else -1, mi_last_error set).  While on, a load in MI_AUG_RRC mode launches the antialiased kernel (virt = the
 * input size, window 0) in place of the bilinear one: same plan, same stream, under prefetch and rank slices alike; every other mode is
 * untouched.  Off by default, and then every launch and bit is what it was.  A batch prefetched under the other choice is dropped.  Not dumped. */
int mi_batch_set_antialias(Batch *b, int on);
/* mi_trainer_eval_u8 with the centre crop replaced by torchvision's Resize(resize) + CenterCrop(input) on bytes: every whole image scaled
 * to resize x resize by the antialiased kernel, of which the window at offset (resize - input) / 2 (integer quotient) on both axes is
 * scored.  dim_in may be smaller than the input (an upscale).  resize == dim_in gives mi_trainer_eval_u8's records bit for bit.
 * -1 as mi_trainer_eval_u8 and for resize < input; it shares that call's scratch and honours mi_trainer_eval_use_ema alike. */
int mi_trainer_eval_u8_resized(Train_ResNet *t, const uint8_t *images_host, const int *labels_host, int64_t n, int dim_in, int resize, int topk,
                               MiLossMetrics *out);

/* ---------------- mixing: mixup and CutMix in place, a two-label loss head ----------------
 * mixup (Zhang et al. 2018) blends every image of a batch with a partner, CutMix (Yun et al. 2019) pastes a box of the partner into it;
 * the loss weighs both images' labels.  The partner of row i is row n - 1 - i (timm's x.flip(0)), one weight lam and one box per batch.
 * Everything here is off by default, and with nothing enabled every launch, value and dumped file is what it was.
 *
 * mi_mix_plan: host-only and deterministic, a pure function of its arguments.  mode 0 none (lam = 1.f), 1 mixup, 2 CutMix; the box is
 * rows [y0, y1) x columns [x0, x1) (all 0 unless mode 2).  s = splitmix64_at(seed, epoch), k = splitmix64_at(s, step world + rank)
 * (the index modulo 2^64), d(j) = splitmix64_at(k, j), U(x) = (x >> 11) 2^-53 (the counter streams of synth.c, as the RRC plan):
 *   U(d(0)) >= prob: mode 0.  Else with both alphas > 0: U(d(1)) < switch_prob picks CutMix, else mixup; with one alpha > 0 that mode.
 *   lam ~ Beta(alpha, alpha), alpha the chosen mode's, by Johnk's method: try t = 0 .. 63: X = pow(U(d(2 + 2t)), 1 / alpha), Y = pow(U(d(3 +
 *   2t)), 1 / alpha); the first try with 0 < X + Y <= 1 gives lam = X / (X + Y); no try taken: lam = 0.5.
 *   CutMix (timm's rand_bbox on a D x D image, D = dim): cut = (int)(D sqrt(1 - lam)), cy = ((d(130) >> 32) D) >> 32, cx likewise from
 *   d(131), y0 = clamp(cy - cut / 2, 0, D), y1 = clamp(cy + cut / 2, 0, D) (cut / 2 the integer quotient), x0, x1 likewise; then
 *   lam = 1 - (double)((y1 - y0) (x1 - x0)) / (D D).
 * Plain double arithmetic, every operation rounded on its own (1 / alpha included); lam is that double rounded to float once.
 * Returns 0, or -1 with mi_last_error set: an alpha outside [0, 1] (0 = that mode off; Johnk's acceptance rate falls off above 1; the
 * recipes use 0.2, 0.8 and 1.0), both alphas 0, prob or switch_prob outside [0, 1], dim outside [1, 16384], rank outside [0, world). */
typedef struct { int mode; float lam; int y0, x0, y1, x1; } MiMixPlan;
int mi_mix_plan(uint64_t seed, int epoch, int64_t step, int rank, int world, double mixup_alpha, double cutmix_alpha, double prob,
                double switch_prob, int dim, MiMixPlan *out);
/* the mix kernels on their own (kernels_input.hip): images_nchw fp32 [n][3][dim][dim] in device memory, mixed IN PLACE, row i with row
 * n - 1 - i; for odd n the middle row is not touched.  plan_host: a MiMixPlan in host memory.
 *   mode 1: a' = (lam (x) a) (+) (mu (x) b), b' = (lam (x) b) (+) (mu (x) a), mu = 1.f - lam, (x) and (+) fp32 operations rounded one by one
 *           (no fused multiply-add): the bits of a float32 numpy model.  lam = 1.f leaves every value (-0.f becomes +0.f beside a finite
 *           partner, a non-finite partner makes NaN: 0 (x) inf).  16-byte accesses where image_size % 4 == 0 and images is 16-byte aligned.
 *   mode 2: inside rows [y0, y1) x columns [x0, x1) of every plane a and b change places, bit for bit; the box is clamped on the
 *           device (y0 into [0, dim], y1 into [y0, dim], x likewise): nothing outside it is read or written, an empty box launches nothing.
 *   mode 0: nothing is launched.
 * Returns 0, or -1 with mi_last_error set and nothing launched: n outside [1, 65535], image_size != 3 dim^2, dim outside [1, 16384], a NULL
 * pointer, images not 4-byte aligned, an unknown mode, mode 1 with lam outside [0, 1]. */
int mi_op_mix_batch(float *images_nchw, int n, int image_size /* 3 dim^2 */, int dim, const MiMixPlan *plan_host);
/* host only, launches nothing: [0] threads of a workgroup, [1] the cap on grid.x, [2] waves of a workgroup.  One sweep of the capped grid
 * covers [0] [1] work items of a pair in mode 1 (16-byte groups, or elements) and [1] [2] row segments of a box in mode 2 */
void mi_debug_mix_geometry(size_t out[3]);
/* the two-label head: mi_op_loss_head with labels a (the image's own) and b (its partner's) per row and one weight lam in [0, 1].  With
 * u = eps / (float)L, wa = (1.f - eps) (x) lam, wb = (1.f - eps) (x) (1.f - lam), each product rounded once:
 *   pred      the bits of mi_op_softmax
 *   dlogits   p_j - t_j, t_j = w_j (+) u, w_j = (j == a ? wa : 0.f) (+) (j == b ? wb : 0.f), in that order: at lam = 1.f that is (1.f - eps)
 *             + u on a and u elsewhere, the bits of mi_op_loss_head, whatever labels_b holds
 *   row_loss  logf(s) - wa z_a - wb z_b - u sum_j z_j (rows longer than 1024 keep the double lane sums); the bound of mi_op_loss_head,
 *             2^-19 (2 + ref), holds against the two-label float64 value ("Loss head")
 *   row_rank  measured against label a alone.  On a mixed batch it says whether the image's own class still leads: a training-time
 *             indicator, not an accuracy
 * a outside [0, L): as mi_op_loss_head (no t_a term, rank L, loss NaN).  b outside [0, L) with wb > 0: no t_b term, row_loss = NaN; with
 * wb == 0 labels_b is not read.  Nothing outside the row is read.  The reduce launch and the records are mi_op_loss_head's.  Returns 0,
 * or -1 as mi_op_loss_head, and for lam outside [0, 1] or labels_b NULL. */
int mi_op_loss_head_mix(const float *logits, const int *labels_a, const int *labels_b, float lam, float *pred, float *dlogits, float *row_loss,
                        int *row_rank, int N, int L, float smoothing, int topk, MiLossMetrics *last_dev, MiLossMetrics *total_dev);
/* The trainer.  While mixing is on load_new_batch ends, for every data source and behind the prefetch swap, on the compute stream, with:
 * the plan of (seed, cur_epoch, cur_dump_id before its increment, the Batch's rank and world: mi_batch_set_rank_slice) -- values a dump
 * saves, so a resumed run and a prefetching run see the same draws --, the mix launch on Batch.images (dim = the network's input), and
 * one launch that writes labels_b[i] = labels[n - 1 - i] into an array of the trainer's; forward_pass then runs the two-label head with
 * that array and the plan's lam (mode 0: the one-label head, no other launch).  correct_classes keeps the images' own labels, and
 * mi_trainer_metrics' top-1 / top-k counts are measured against them.  backwards_pass is unchanged.  The eval entry points never mix;
 * mi_trainer_eval_forward on the CURRENT batch (Batch.images) sees the mixed pixels.  Refused (-1, mi_last_error set) unless the head
 * is MI_LOSS_DEVICE, and for arguments mi_mix_plan refuses; mi_trainer_set_loss in turn refuses to drop MI_LOSS_DEVICE while mixing is
 * on.  Both alphas 0 switch it off.  May be called between steps.  Like the optimizer and the loss setting it is not dumped: a
 * resumed run sets it again.  mi_trainer_last_mix: the plan of the last load_new_batch (all 0 before the first); -1 while mixing is off. */
int mi_trainer_set_mix(Train_ResNet *t, double mixup_alpha, double cutmix_alpha, double prob, double switch_prob, uint64_t seed);
int mi_trainer_last_mix(const Train_ResNet *t, MiMixPlan *out);

/* ---------------- random erasing: a box per image, filled in place with a constant or with noise ----------------
 * Random erasing (Zhong et al. 2017; torchvision's RandomErasing, timm's --reprob) overwrites one box of an image.  It is a per-sample
 * transform: every row of the batch has its own draw, and the labels do not change.  Off by default; with it off every launch, value and
 * dumped file is what it was.
 *
 * mi_erase_plan: host-only and deterministic, a pure function of its arguments.  out[4 i ..] = (y0, x0, h, w) of row i, all 0 for a row
 * that is not erased; h == 0 or w == 0 means no box.  s = splitmix64_at(seed, epoch), k = splitmix64_at(s, step world + rank) (modulo
 * 2^64: mi_mix_plan's step key), e = splitmix64_at(k, 1000) (the mix plan draws indices up to 131 from k: equal seeds share no draw),
 * k_i = splitmix64_at(e, i), d(j) = splitmix64_at(k_i, j), U(x) = (x >> 11) 2^-53.  torchvision's RandomErasing.forward + get_params
 * on a D x D image, D = dim:
 *   U(d(0)) >= prob: no box.  Else try t = 0 .. 9: target = D D (scale_lo + U(d(1 + 4t)) (scale_hi - scale_lo)), ratio = exp(log(ratio_lo) +
 *   U(d(2 + 4t)) (log(ratio_hi) - log(ratio_lo))), h = lrint(sqrt(target ratio)), w = lrint(sqrt(target / ratio)) (half to even; h takes the
 *   product, the other way round than the RRC plan: torchvision's own asymmetry); the first try with h < D and w < D (strict) is taken:
 *   y0 = ((d(3 + 4t) >> 32) (D - h + 1)) >> 32, x0 = ((d(4 + 4t) >> 32) (D - w + 1)) >> 32.  No try taken: no box (torchvision returns the
 *   image).  At tiny D a taken try may have h == 0 or w == 0: a legal, empty box, stored as drawn.
 * Plain double arithmetic, every operation rounded on its own.  Returns 0, or -1 with mi_last_error set: n < 0, dim outside [1, 16384],
 * prob outside [0, 1], scale_lo or ratio_lo not positive, scale_hi < scale_lo, ratio_hi < ratio_lo, rank outside [0, world). */
int mi_erase_plan(uint64_t seed, int epoch, int64_t step, int rank, int world, int n, int dim, double prob, double scale_lo, double scale_hi,
                  double ratio_lo, double ratio_hi, int *out);
/* the erase kernel on its own (kernels_input.hip): images_nchw fp32 [n][3][dim][dim] in device memory, IN PLACE; boxes_host int [n][4]
 * (y0, x0, h, w) and fill_host in host memory, both read before the call returns.  Every box is clamped (y0 into [0, dim], h into
 * [0, dim - y0], x likewise; on the host and again on the device); nothing outside a row's box is read or written, and every word
 * outside the boxes keeps its bits.  A row without a box writes nothing; a launch none of whose rows has a box is skipped.
 *   MI_ERASE_CONST: every element of plane c in the box becomes value[c].
 *   MI_ERASE_NOISE: element (c, y, x) of row i becomes value[c] (+) std[c] (x) z, product and sum fp32 operations rounded one by one.  z
 *     depends on the element's POSITION only, not on the box or the launch: q = splitmix64_at(noise_seed, first_row + i), el = (c dim + y)
 *     dim + x, g_m = splitmix64_at(q, 64 + 3 el + m) for m = 0, 1, 2, S = the sum of the twelve 16-bit fields (g_m >> 16 f) & 0xFFFF,
 *     f = 0 .. 3, z = (float)(S - 393210) 2^-16 (exact).  That is the Irwin-Hall approximation of a unit normal: mean 0, variance
 *     1 - 2^-32, |z| < 6 -- NOT Gaussian in the tails.  It is integer arithmetic, so device, numpy model and any port agree bit for bit.
 * The boxes reach the device as kernel arguments, four uint16 a row, 256 rows a launch: no staging buffer, no copy, no event.  16-byte
 * stores where image_size % 4 == 0 and images is 16-byte aligned.  Returns 0, or -1 with mi_last_error set and nothing launched: a NULL
 * pointer, n outside [1, 65535], dim outside [1, 16384], image_size != 3 dim^2, images not 4-byte aligned, an unknown mode, a value or std
 * that is not finite, a negative std. */
enum { MI_ERASE_CONST = 0, MI_ERASE_NOISE = 1 };
typedef struct { int mode; float value[3]; float std[3]; uint64_t noise_seed; } MiEraseFill;
int mi_op_erase_batch(float *images_nchw, int n, int image_size /* 3 dim^2 */, int dim, const int *boxes_host /* [n][4] */,
                      const MiEraseFill *fill_host, int64_t first_row /* row i uses noise key index first_row + i */);
/* host only, launches nothing: [0] threads of a workgroup, [1] the cap on grid.x, [2] waves of a workgroup, [3] rows of a launch.  One
 * sweep of the capped grid covers [1] [2] row segments of a row's box */
void mi_debug_erase_geometry(size_t out[4]);
/* The trainer.  While erasing is on load_new_batch ends, for every data source and behind the prefetch swap, on the compute stream and IN
 * FRONT OF the mix step (erasing is a per-sample transform, mixing the collate step), with: the plan of (seed, cur_epoch, cur_dump_id
 * before its increment, the Batch's rank and world) for batch_size rows at dim = the network's input -- the values the mix step uses, so
 * a resumed run and a prefetching run see the same boxes --, and the erase launch on Batch.images with noise_seed = the plan's e and
 * first_row = 0 (fill->noise_seed is ignored).  Either loss head; no label changes; the eval entry points never erase.  prob == 0
 * switches it off; with it off nothing is launched and nothing allocated.  May be called between steps.  Like the optimizer and the mix
 * setting it is not dumped: a resumed run sets it again.  Refused (-1, mi_last_error set) for arguments mi_erase_plan or
 * mi_op_erase_batch refuses.  mi_trainer_last_erase: the boxes of the last load_new_batch into out [batch_size][4]; returns the rows
 * written (0 before the first load), -1 while erasing is off. */
int mi_trainer_set_erase(Train_ResNet *t, double prob, double scale_lo, double scale_hi, double ratio_lo, double ratio_hi,
                         const MiEraseFill *fill /* noise_seed ignored */, uint64_t seed);
int mi_trainer_last_erase(const Train_ResNet *t, int *out /* [batch_size][4] */);

/* ---------------- TrivialAugmentWide: one of 14 Pillow operations per image, at one of 31 strengths, in place ----------------
 * TrivialAugmentWide (Mueller & Hutter 2021; torchvision's --auto-augment ta_wide) draws, per image, one operation uniformly and one of
 * 31 strength bins uniformly, and a sign for the signed operations.  torchvision applies it to the PIL image (bytes) in front of the
 * normalisation; here it runs on the fp32 batch behind the decode: per pixel the contract is decode o Pillow-op o quantise, and the
 * result is, bit for bit, what applying Pillow's operation to the cropped bytes and decoding them gives (tests/taref.py restates the
 * arithmetic and is pinned to Pillow itself).  Off by default; with it off every launch, value and dumped file is what it was.
 *
 * The operations, in torchvision's dictionary order, and their magnitudes at bin b (torchvision's _augmentation_space(31): float32
 * torch.linspace values widened to double, committed as tables in loader.c):
 *   SHEAR_X, SHEAR_Y, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS   linspace(0, 0.99, 31)[b], signed
 *   TRANSLATE_X, TRANSLATE_Y                                   linspace(0, 32, 31)[b], signed (not b 32 / 30: int() of it is 0 .. 15, 17 .. 30, 32)
 *   ROTATE                                                     4.5 b degrees, signed
 *   POSTERIZE                                                  8 - round(b / 5) bits (8 .. 2), unsigned
 *   SOLARIZE                                                   255 - 8.5 b, unsigned
 *   IDENTITY, AUTOCONTRAST, EQUALIZE                           none
 *
 * mi_ta_row: host-only, a pure function; fills the record of (op, bin, neg) on a dim x dim image in double arithmetic, every operation
 * rounded on its own.  neg is ignored (stored as 0) by the unsigned operations.
 *   magnitude  the signed magnitude m (the bits for POSTERIZE, the threshold for SOLARIZE, 0 where there is none)
 *   factor     (float)(1.0 + m) for BRIGHTNESS, COLOR, CONTRAST, SHARPNESS: Pillow's ImageEnhance factor, a C float in Image.blend; else 0
 *   arg        POSTERIZE: the mask ~(2^(8 - bits) - 1) & 255; SOLARIZE: ceil(threshold), since i < threshold on integers; else 0
 *   A[6]       the five geometric operations: Pillow's 16.16 fixed-point coefficients of the inverse matrix (a0 .. a5), FIX(v) = floor(v 65536
 *              + 0.5): A0 = FIX(a0), A1 = FIX(a1), A3 = FIX(a3), A4 = FIX(a4), A2 = FIX(a2 + a0 / 2 + a1 / 2), A5 = FIX(a5 + a3 / 2 + a4 / 2);
 *              else 0.  The matrices are torchvision's for PIL images:
 *                SHEAR_X (1, t, 0, 0, 1, 0), SHEAR_Y (1, 0, 0, t, 1, 0), t = tan(radians(degrees(atan(m)))) (centre: the top-left corner);
 *                TRANSLATE_X a2 = -int(m), TRANSLATE_Y a5 = -int(m) (int truncates toward zero), the rest of the identity;
 *                ROTATE by m degrees, Pillow's Image.rotate(m, NEAREST) about (dim / 2, dim / 2): r = -radians(m mod 360) (the sign of
 *                the divisor, as Python's %), a0 = a4 = round(cos r, 15), a1 = round(sin r, 15), a3 = round(-sin r, 15) (decimal
 *                places, half to even on the exact value), a2 = a0 (-dim / 2) + a1 (-dim / 2) + dim / 2, a5 likewise from a3, a4.
 *                +-90 degrees comes out of this route as Pillow's transpose: there is no special case.
 * Returns 0, or -1 with mi_last_error set: out NULL, op outside [0, 14), bin outside [0, 31), neg not 0 or 1, dim outside [1, 4096]
 * (every 32-bit sum of the gather below then stays under 2^31: DESIGN.md, "Size limits").
 *
 * mi_ta_plan: host-only and deterministic, the erase plan's scheme under a key of its own.  s = splitmix64_at(seed, epoch), k =
 * splitmix64_at(s, step world + rank) (modulo 2^64: mi_mix_plan's step key), a = splitmix64_at(k, 2000) (the mix plan draws indices up to
 * 131 from k, the erase plan index 1000: equal seeds share no draw), k_i = splitmix64_at(a, i), d(j) = splitmix64_at(k_i, j):
 * op = ((d(0) >> 32) 14) >> 32, bin = ((d(1) >> 32) 31) >> 32, neg = d(2) >> 63; out[i] = mi_ta_row(op, bin, neg, dim).  Returns 0, or -1
 * with mi_last_error set: n < 0, out NULL with n > 0, dim outside [1, 4096], rank outside [0, world).
 *
 * mi_op_trivial_augment (kernels_input.hip): images_nchw fp32 [n][3][dim][dim] in device memory, IN PLACE; rows_host [n] in host memory,
 * read before the call returns; workspace_dev: mi_ta_workspace_bytes(n, dim) bytes of device memory, 16-byte aligned, contents
 * arbitrary (the integer statistics [n][4][256] are zeroed on the stream, then a planar uint8 staging area [n][3][dim][dim]).  No
 * synchronisation and no host round trip: the records travel as kernel arguments, 128 rows a launch, two launches per 128 rows.
 *   quantise  b = (int)rint(clamp(v (+) mean_plane, 0, 255)): one fp32 addition, NaN gives 0, half to even.  mean_plane is the fp32 of
 *             the mean the decode table subtracts on that plane (plane d holds source position 2 - d: the R plane carries 103.94).  For
 *             every byte-valued source -- fp32 shards, uint8 shards under fixed / centre / random crops, the antialiased random-resized
 *             crop -- this recovers the byte exactly; other sources (the 8-bit bilinear resample, synthetic batches) are ROUNDED to the
 *             nearest byte, as conversion to a PIL image would do.
 *   decode    the decode table's value of the result byte: (float)((double)(float)b - mean).
 *   Rows with MI_TA_IDENTITY are neither read nor written: every word keeps its bits.  Draws that happen to be numerically neutral
 *   (POSTERIZE at 8 bits, a zero shear) are not special-cased: they quantise and decode.
 *   blend(d, x, f) = d (+) f (x) (x (-) d) in fp32, every operation rounded on its own (no FMA); for 0 <= f <= 1 the result is (int)t, else 0
 *   where t <= 0, 255 where t >= 255, (int)t elsewhere: Pillow's ImagingBlend.  L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16.
 *   BRIGHTNESS blend(0, i, f).  CONTRAST blend(M, i, f), M = (2 sum(L) + D^2) / (2 D^2) in 64-bit integers (Pillow's int(mean + 0.5)).
 *   COLOR blend(L, x, f).  SHARPNESS blend(S, x, f), S = ImageFilter.SMOOTH of the channel: 0.5f plus the nine products with (float)(1 /
 *   13.) (centre (float)(5 / 13.)) added in row-major order, one rounding each, clipped as above; the outermost rows and columns are
 *   the source.  POSTERIZE i & arg.  SOLARIZE i < arg ? i : 255 - i.  AUTOCONTRAST per channel from the lowest and highest occupied
 *   bin: hi <= lo leaves the channel; else scale = 255.0 / (hi - lo), off = -lo scale, clamp((int)(i scale + off), 0, 255) in double,
 *   product and sum rounded separately, truncation toward zero.  EQUALIZE per channel: step = (D^2 - h[last occupied]) / 255; fewer than
 *   two occupied bins or step == 0: the identity; else n = step / 2, and for i = 0 .. 255 the entry is min(255, n / step), then n += h[i].
 *   The geometric operations: xin = (A2 + A1 y + A0 x) >> 16, yin = (A5 + A4 y + A3 x) >> 16 (arithmetic shifts); the source byte where
 *   both lie inside the image, byte 0 elsewhere (torchvision's fill = None).
 * Returns 0, or -1 with mi_last_error set and nothing launched: a NULL pointer, n outside [1, 65535], dim outside [1, 4096], image_size
 * != 3 dim^2, images not 4-byte aligned or workspace not 16-byte aligned, an op or bin out of range. */
enum { MI_TA_IDENTITY = 0, MI_TA_SHEAR_X, MI_TA_SHEAR_Y, MI_TA_TRANSLATE_X, MI_TA_TRANSLATE_Y, MI_TA_ROTATE, MI_TA_BRIGHTNESS, MI_TA_COLOR,
       MI_TA_CONTRAST, MI_TA_SHARPNESS, MI_TA_POSTERIZE, MI_TA_SOLARIZE, MI_TA_AUTOCONTRAST, MI_TA_EQUALIZE, MI_TA_OPS = 14, MI_TA_BINS = 31 };
typedef struct { int op, bin, neg, arg; double magnitude; float factor; int A[6]; } MiTaRow;
int mi_ta_row(int op, int bin, int neg, int dim, MiTaRow *out);
int mi_ta_plan(uint64_t seed, int epoch, int64_t step, int rank, int world, int n, int dim, MiTaRow *out);
size_t mi_ta_workspace_bytes(int n, int dim);
int mi_op_trivial_augment(float *images_nchw, int n, int image_size /* 3 dim^2 */, int dim, const MiTaRow *rows_host, void *workspace_dev);
/* host only, launches nothing: [0] threads of a workgroup, [1] the cap on grid.x, [2] rows of a launch, [3] pixels a thread takes per
 * turn on the 16-byte path (1 on the other).  One sweep of the capped grid covers [0] [1] ([3]) pixels of an image */
void mi_debug_ta_geometry(size_t out[4]);
/* The trainer.  While it is on load_new_batch runs, for every data source and behind the prefetch swap, on the compute stream and IN
 * FRONT OF the erase step (the order is augment, erase, mix): the plan of (seed, cur_epoch, cur_dump_id before its increment, the Batch's
 * rank and world) for batch_size rows at dim = the network's input -- the step key the erase and mix plans use --, and the launches
 * of mi_op_trivial_augment on Batch.images.  The workspace is allocated at the first call with on != 0; with it off nothing is
 * launched and nothing allocated.  The eval entry points never augment.  May be called between steps.  Like the erase and mix
 * settings it is not dumped: a resumed run sets it again.  Refused (-1, mi_last_error set): an input above 4096.
 * mi_trainer_last_trivial_augment: the records of the last load_new_batch into out [batch_size]; returns the rows written (0 before
 * the first load), -1 while it is off. */
int mi_trainer_set_trivial_augment(Train_ResNet *t, int on, uint64_t seed);
int mi_trainer_last_trivial_augment(const Train_ResNet *t, MiTaRow *out /* [batch_size] */);

/* typed operator layer: x_dt = storage type of the convolution-side tensors (x, dx), a_dt = of the activation-side tensors
 * (y, residual, dy, mask_src, gated_out).  Supported pairs: (F32,F32), (BF16,BF16), (F32,BF16). */
int mi_op_convert(const void *in, int in_dt, void *out, int out_dt, size_t n);
int mi_bf16_conv_supported(int op, int N, int C, int H, int K, int k, int stride); /* op 0 fwd, 1 dgrad, 2 wgrad */
int mi_bf16_pw_wgrad_supported(int N, int C, int H, int K); /* 1: this 1x1 weight gradient runs on the LDS-DMA kernel (both operands as they lie) */
int mi_op_conv_fwd_bf16(const void *x_bf16, const float *w_kcrs, void *y_bf16, int N, int C, int H, int K, int k, int stride);
int mi_op_conv_dgrad_bf16(const float *w_kcrs, const void *dy_bf16, void *dx_bf16, int N, int C, int H, int K, int k, int stride,
                          int to_add);
int mi_op_conv_wgrad_bf16(const void *x_bf16, const void *dy_bf16, float *dw_kcrs, int N, int C, int H, int K, int k, int stride);
/* prepreAndDoConvolutionDeriv + activationAndBatchNormDeriv as backwards_pass chains them in bf16 storage (resnet.cu:1399-1429,
 * 1455-1480): dgrad of a convolution, then the backward of the batch norm (+ReLU, gate = mask > 0) in front of it; where the launch
 * allows the dgrad does the BN' reduction pass in its epilogue.  gated = (mask > 0 ? dgrad(+addend) : 0), bn_dx = the BN's input
 * gradient.  Image tensors bf16.  Returns < 0 on error, else the number of partial rows the dgrad left (0 = separate pass). */
int mi_op_conv_dgrad_bn_bwd_bf16(const float *w_kcrs, const void *dy, const void *addend, void *gated, int N, int C, int H, int K, int k,
                                 int stride, const void *bn_x, const void *mask, const float *gamma, const float *beta, const float *means,
                                 const float *vars, float eps, void *bn_dx, float *dgamma, float *dbeta);
/* 3x3 convolutions of the bf16 path on channel-last, zero-padded operands (round 3; kernels_cl_bf16.hip): the operand is re-laid once
 * (one plane with a halo of 1, or four parity planes for stride 2), both MFMA operands then go global -> LDS by LDS-DMA.  Same tensors
 * and semantics as mi_op_conv_fwd_bf16 / mi_op_conv_dgrad_bf16 with k = 3; -2: shape not covered (channels % 64) */
int mi_op_conv_fwd_bf16_cl(const void *x_bf16, const float *w_kcrs, void *y_bf16, int N, int C, int H, int K, int stride);
int mi_op_conv_wgrad_bf16_cl(const void *x_bf16, const void *dy_bf16, float *dw_kcrs, int N, int C, int H, int K, int stride); /* C % 128, K % 128, plane % 4 */
int mi_op_bn_fwd_cl_bf16(const void *x_bf16, const float *gamma, const float *beta, const void *residual_bf16, float *means, float *vars, void *y_bf16, void *y_cl, int N, int C, int H, float eps, int par); /* BN (+ residual) + ReLU written twice: NCHW and channel-last (par 0: one zero-padded plane [N][H+2][H+2][C]; par 1: the four parity planes of a stride-2 3x3; interior only; C % 64) */
int mi_op_conv1x1_fwd_bf16_cl(const void *x_bf16, const float *w_kc, void *y_bf16, int N, int C, int H, int K); /* 1x1 forward on the input re-laid dense channel-last (one tap of the channel-last kernel); C, K % 64 */
int mi_op_conv_wgrad_bf16_cl2(const void *x, const void *dy, float *dw, int N, int C, int H, int K, int stride); /* 3x3: BOTH operands as channel-last planes (stride 2: the input's parity planes and the dY planes of the stride-2 dgrad; stride 1: both with a halo of 1); C, K % 128, any plane size */
int mi_op_conv_dgrad_bf16_cl(const float *w_kcrs, const void *dy_bf16, void *dx_bf16, int N, int C, int H, int K, int stride, int to_add); /* stride 2: C % 128, no to_add */
/* the same chain in fp32 storage: dgrads with stride 1 on the MFMA implicit-GEMM route do the reduction in their epilogue.  Image tensors
 * fp32.  Returns < 0 on error, else the number of partial rows the dgrad left (0 = separate pass). */
int mi_op_conv_dgrad_bn_bwd_f32(const float *w_kcrs, const float *dy, const float *addend, float *gated, int N, int C, int H, int K, int k,
                                int stride, const float *bn_x, const float *mask, const float *gamma, const float *beta, const float *means,
                                const float *vars, float eps, float *bn_dx, float *dgamma, float *dbeta);
/* the stem convolution of the bf16 storage mode (7x7 stride 2, 3 -> 64 filters, H a multiple of 32; doConvolution /
 * convolutionDerivWeights, resnet.cu:109-156, 227-281): fp32 tensors in and out, image and weights rounded to bf16 inside,
 * fp32 accumulation on the bf16 matrix cores.  -2: shape not covered (the trainer then keeps the fp32 stem). */
int mi_op_stem_fwd_bf16(const float *x, const float *w_kcrs, float *y, int N, int H);
int mi_op_stem_wgrad_bf16(const float *x, const float *w_kcrs, const float *dy, float *dw_kcrs, int N, int H);
/* the same stem in exact fp32 arithmetic on the fp32 matrix cores (what the fp32 trainer runs unless RESNET_MI_IGEMM=0) */
int mi_op_stem_fwd_f32(const float *x, const float *w_kcrs, float *y, int N, int H);
int mi_op_stem_wgrad_f32(const float *x, const float *w_kcrs, const float *dy, float *dw_kcrs, int N, int H);
/* prepareAndDoConvolution + prepareAndDoBatchNormAndActivate as forward_pass pairs them (resnet.cu:1386-1396, 1431-1453): BN
 * statistics from the convolution's own epilogue where the layer runs on the implicit GEMM.  dt = storage type of x, conv_out, y.
 * Returns < 0 on error, else the number of statistics partial rows the convolution left (0 = separate statistics pass). */
int mi_op_conv_bn_fwd_t(const void *x, const float *w_kcrs, void *conv_out, int dt, const float *gamma, const float *beta,
                        float *means, float *vars, void *y, int N, int C, int H, int K, int k, int stride, float eps, int relu);
/* the same pair on the channel-last 3x3 forward (the bf16 trainer's route for 3x3 layers with channels % 64): x, conv_out, y bf16.
 * -2: shape not covered; else < 0 on error, or the number of statistics partial rows the convolution left */
int mi_op_conv_bn_fwd_bf16_cl(const void *x_bf16, const float *w_kcrs, void *conv_out_bf16, const float *gamma, const float *beta,
                              float *means, float *vars, void *y_bf16, int N, int C, int H, int K, int stride, float eps, int relu);
/* the stem (7x7 stride 2, 3 -> 64) and its BN + ReLU on the matrix cores: exact = 1 the fp32 trainer's (conv_dt fp32), exact = 0 the bf16
 * trainer's with conv_out stored as conv_dt (fp32 or bf16); y stored as a_dt.  Returns as mi_op_conv_bn_fwd_t. */
int mi_op_stem_bn_fwd_t(const float *x, const float *w_kcrs, void *conv_out, int conv_dt, const float *gamma, const float *beta,
                        float *means, float *vars, void *y, int a_dt, int N, int H, float eps, int exact);
/* the bf16 stem's weight gradient from dy stored as dy_dt (fp32 or bf16) */
int mi_op_stem_wgrad_bf16_t(const float *x, const float *w_kcrs, const void *dy, int dy_dt, float *dw_kcrs, int N, int H);
int mi_op_bn_fwd_t(const void *x, int x_dt, const float *gamma, const float *beta, const void *residual, float *means, float *vars,
                   void *y, int a_dt, int N, int C, int H, float eps, int relu);
int mi_op_bn_apply_t(const void *x, int x_dt, const float *gamma, const float *beta, const void *residual, const float *means,
                     const float *vars, void *y, int a_dt, int N, int C, int H, float eps, int relu);
int mi_op_bn_bwd_t(const void *x, int x_dt, const float *gamma, const float *beta, const float *means, const float *vars,
                   const void *dy, const void *mask_src, void *gated_out, int a_dt, void *dx, float *dgamma, float *dbeta, int N, int C,
                   int H, float eps, int mask_mode);
int mi_op_maxpool_fwd_t(const void *x, void *y, int dt, int *max_inds, int N, int C, int H, int k, int stride);
int mi_op_maxpool_bwd_t(const int *max_inds, const void *dy, void *dx, int dt, int N, int C, int H, int k, int stride);
int mi_op_avgpool_fwd_t(const void *x, int dt, float *y, int N, int C, int H);
int mi_op_avgpool_bwd_t(const float *dy, void *dx, int dt, int N, int C, int H);

#ifdef __cplusplus
}
#endif
#endif
