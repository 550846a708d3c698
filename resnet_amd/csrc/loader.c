/*
 * loader.c -- Batch state and load_new_batch (resnet.cu:1196-1325) plus class metadata (resnet.cu:1328-1381).
 * The reference keeps a whole shard in host RAM, memcpy's one batch into pinned memory and does a blocking
 * H2D copy; shard files are raw fp32 images + int32 labels (build_training_shards.c:150-160), NHWC in the
 * legacy directory and NCHW under nchw/.  Same behaviour here, with the data source selectable (shards,
 * a dumped images.buffer/labels.buffer pair, caller-filled host buffers, or a seeded synthetic pool that
 * stays resident in HBM) because the reference's /mnt/storage paths are literals.
 * MI_SRC_SHARDS_U8 (new work, no counterpart in the reference): the shard holds whole uint8 images; the crop is drawn per load by
 * mi_augment_plan and made, with the flip and the float conversion, by the decode kernel (kernels_input.hip).  MI_AUG_RRC: the plan
 * is a box per image (mi_augment_plan_rrc) and the resample kernel scales it to the input size -- the two-tap bilinear one, or with
 * mi_batch_set_antialias the one that filters as Pillow does.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_host.h"
#include "mi_aa.h"

static BatchExt *g_ext = NULL;
BatchExt *mi_batch_ext(Batch *b) {
    for (BatchExt *e = g_ext; e; e = e->next) if (e->batch == b) return e;
    BatchExt *e = (BatchExt *)calloc(1, sizeof(BatchExt));
    e->batch = b; e->source = MI_SRC_SHARDS; e->layout = MI_LAYOUT_NCHW; e->world = 1;
    e->shard_dir = strdup("/mnt/storage/data/vision/imagenet/2012/train_data_shards"); /* resnet.cu:1275 */
    e->next = g_ext; g_ext = e;
    return e;
}
void mi_batch_ext_free(Batch *b) {
    if (!b) return;
    BatchExt **pp = &g_ext;
    while (*pp && (*pp)->batch != b) pp = &(*pp)->next;
    if (*pp) {
        BatchExt *e = *pp;
        *pp = e->next;
        free(e->shard_dir); free(e->images_path); free(e->labels_path);
        mid_free(e->pool_images); mid_free(e->pool_labels); mid_free(e->stage_dev); free(e->pool_labels_host);
        mid_free(e->images_next); mid_free(e->stage_next); mid_free(e->labels_next);
        mid_free_host(e->pinned_next); mid_free_host(e->labels_next_host);
        if (e->ev_next) mid_event_destroy(e->ev_next);
        if (e->ev_compute) mid_event_destroy(e->ev_compute);
        free(e->u8_shard); free(e->u8_crops);
        for (int k = 0; k < 2; k++) {
            mid_free_host(e->u8_pinned[k]); mid_free(e->u8_dev[k]); mid_free_host(e->plan_pinned[k]); mid_free(e->plan_dev[k]);
        }
        free(e);
    }
    mid_free_host(b->images_float_cpu); mid_free_host(b->correct_classes_cpu);
    mid_free(b->images); mid_free(b->correct_classes);
    free(b->full_shard_images); free(b->full_shard_correct_classes);
    free(b);
}

/* resnet.cu:1196-1231.  The shard-sized host buffers are allocated at the first shard load. */
Batch *init_general_batch(int n_images, int image_size, int image_dim, int shard_n_images) {
    Batch *b = (Batch *)calloc(1, sizeof(Batch));
    b->n_images = n_images; b->image_size = image_size; b->image_dim = image_dim;
    b->images_float_cpu = (float *)mid_malloc_host((size_t)n_images * image_size * sizeof(float));
    b->images = (float *)mid_malloc((size_t)n_images * image_size * sizeof(float));
    b->correct_classes_cpu = (int *)mid_malloc_host((size_t)n_images * sizeof(int));
    b->correct_classes = (int *)mid_malloc((size_t)n_images * sizeof(int));
    b->cur_shard_id = -1; b->cur_batch_in_shard = -1; b->shard_n_images = shard_n_images;
    mi_batch_ext(b);
    return b;
}

static void set_str(char **dst, const char *s) { free(*dst); *dst = s ? strdup(s) : NULL; }
void mi_batch_source_shards(Batch *b, const char *dir, int layout) {
    BatchExt *e = mi_batch_ext(b);
    e->source = MI_SRC_SHARDS; e->layout = layout; set_str(&e->shard_dir, dir);
    e->have_next = 0;
    if (e->prefetch) mi_batch_set_prefetch(b, 1); /* the fp32 staging buffers, should the prefetch have been set up for uint8 shards */
}
/* staging of the uint8 source: set 0 for the blocking load, set 1 for the prefetched batch */
static void u8_ensure(Batch *b, BatchExt *e) {
    const size_t bytes = (size_t)b->n_images * e->u8_dim_in * e->u8_dim_in * 3, plan = (size_t)b->n_images * 5 * sizeof(int);
    for (int k = 0; k < (e->prefetch ? 2 : 1); k++) {
        if (e->u8_pinned[k]) continue;
        e->u8_pinned[k] = (uint8_t *)mid_malloc_host(bytes);
        e->u8_dev[k] = (uint8_t *)mid_malloc(bytes);
        e->plan_pinned[k] = (int *)mid_malloc_host(plan);
        e->plan_dev[k] = (int *)mid_malloc(plan);
    }
}
void mi_batch_source_shards_u8(Batch *b, const char *dir, int image_dim_in) {
    BatchExt *e = mi_batch_ext(b);
    if (e->u8_dim_in != image_dim_in) { /* buffers of another image size */
        free(e->u8_shard); free(e->u8_crops); e->u8_shard = NULL; e->u8_crops = NULL;
        for (int k = 0; k < 2; k++) {
            mid_free_host(e->u8_pinned[k]); mid_free(e->u8_dev[k]); mid_free_host(e->plan_pinned[k]); mid_free(e->plan_dev[k]);
            e->u8_pinned[k] = NULL; e->u8_dev[k] = NULL; e->plan_pinned[k] = NULL; e->plan_dev[k] = NULL;
        }
    }
    e->source = MI_SRC_SHARDS_U8; e->layout = MI_LAYOUT_NCHW; e->u8_dim_in = image_dim_in; set_str(&e->shard_dir, dir);
    e->have_next = 0; e->have_plan = 0;
    u8_ensure(b, e);
}
int mi_batch_set_augment(Batch *b, int mode, int flip, uint64_t seed) {
    BatchExt *e = mi_batch_ext(b);
    if (e->source != MI_SRC_SHARDS_U8) { mi_record_host_error("mi_batch_set_augment", "the data source is not MI_SRC_SHARDS_U8"); return -1; }
    if (mode != MI_AUG_FIXED && mode != MI_AUG_CENTER && mode != MI_AUG_RANDOM) { mi_record_host_error("mi_batch_set_augment", "mode is MI_AUG_FIXED, _CENTER or _RANDOM"); return -1; }
    if (e->aug_mode == MI_AUG_RRC) { /* the last plan is a box plan, and the batch prefetched under it still reads the pinned set */
        e->have_plan = 0;
        if (e->have_next) mid_event_sync(e->ev_next);
    }
    e->aug_mode = mode; e->aug_flip = flip != 0; e->aug_seed = seed;
    e->have_next = 0; /* a batch prefetched under the old choice */
    return 0;
}
int mi_batch_set_augment_rrc(Batch *b, int flip, uint64_t seed, double scale_lo, double scale_hi, double ratio_lo, double ratio_hi) {
    BatchExt *e = mi_batch_ext(b);
    if (e->source != MI_SRC_SHARDS_U8) { mi_record_host_error("mi_batch_set_augment_rrc", "the data source is not MI_SRC_SHARDS_U8"); return -1; }
    if (!(scale_lo > 0) || !(ratio_lo > 0) || !(scale_hi >= scale_lo) || !(ratio_hi >= ratio_lo)) {
        mi_record_host_error("mi_batch_set_augment_rrc", "need 0 < scale_lo <= scale_hi and 0 < ratio_lo <= ratio_hi"); return -1;
    }
    if (e->have_next) mid_event_sync(e->ev_next); /* the batch prefetched under the old choice still reads the pinned set */
    e->aug_mode = MI_AUG_RRC; e->aug_flip = flip != 0; e->aug_seed = seed;
    e->rrc_scale[0] = scale_lo; e->rrc_scale[1] = scale_hi; e->rrc_ratio[0] = ratio_lo; e->rrc_ratio[1] = ratio_hi;
    e->have_next = 0; e->have_plan = 0; /* a batch prefetched under the old choice; a plan of the other shape */
    return 0;
}
int mi_batch_set_antialias(Batch *b, int on) {
    BatchExt *e = mi_batch_ext(b);
    if (e->source != MI_SRC_SHARDS_U8) { mi_record_host_error("mi_batch_set_antialias", "the data source is not MI_SRC_SHARDS_U8"); return -1; }
    if (e->have_next) mid_event_sync(e->ev_next); /* the batch prefetched under the old choice still reads the pinned set */
    e->rrc_antialias = on != 0;
    e->have_next = 0;
    return 0;
}
/* the host's copy of the kernel's tap table (mi_aa.h: the same text) */
int mi_aa_coeffs(int in, int V, int o, int *xmin, int *K, int cap) {
    if (in < 1 || V < 1 || o < 0 || o >= V || !xmin || (!K && cap > 0)) { mi_record_host_error("mi_aa_coeffs", "need in, V >= 1, 0 <= o < V and the two outputs"); return -1; }
    return mi_aa_taps(in, V, o, xmin, K, cap < 0 ? 0 : cap);
}
int mi_batch_last_plan(const Batch *b, int *out) {
    BatchExt *e = mi_batch_ext((Batch *)b);
    if (e->source != MI_SRC_SHARDS_U8 || !e->have_plan || e->aug_mode == MI_AUG_RRC) return -1;
    memcpy(out, e->plan_pinned[0], (size_t)b->n_images * 3 * sizeof(int));
    return b->n_images;
}
int mi_batch_last_boxes(const Batch *b, int *out) {
    BatchExt *e = mi_batch_ext((Batch *)b);
    if (e->source != MI_SRC_SHARDS_U8 || !e->have_plan || e->aug_mode != MI_AUG_RRC) return -1;
    memcpy(out, e->plan_pinned[0], (size_t)b->n_images * 5 * sizeof(int));
    return b->n_images;
}
int mi_augment_plan(int mode, int flip, uint64_t seed, int epoch, int64_t first_global_index, int n, int dim_in, int dim_out,
                    const int *fixed_crops, int *out) {
    const int R = dim_in - dim_out;
    if (R < 0 || dim_out < 1 || n < 0) { mi_record_host_error("mi_augment_plan", "need 1 <= dim_out <= dim_in and n >= 0"); return -1; }
    if (mode == MI_AUG_FIXED) {
        if (!fixed_crops) { mi_record_host_error("mi_augment_plan", "MI_AUG_FIXED needs the shard's crop offsets"); return -1; }
        for (int i = 0; i < n; i++) {
            const int ro = fixed_crops[2 * i], co = fixed_crops[2 * i + 1];
            if (ro < 0 || ro > R || co < 0 || co > R) { mi_record_host_error("mi_augment_plan", "a fixed crop does not fit into the image"); return -1; }
            out[3 * i] = ro; out[3 * i + 1] = co; out[3 * i + 2] = 0;
        }
    } else if (mode == MI_AUG_CENTER) {
        for (int i = 0; i < n; i++) { out[3 * i] = out[3 * i + 1] = R / 2; out[3 * i + 2] = 0; }
    } else if (mode == MI_AUG_RANDOM) {
        const uint64_t s = mi_splitmix64_at(seed, (uint64_t)(int64_t)epoch);
        for (int i = 0; i < n; i++) {
            const uint64_t r = mi_splitmix64_at(s, (uint64_t)(first_global_index + i));
            out[3 * i] = (int)(((r & 0xFFFFF) * (uint64_t)(R + 1)) >> 20);
            out[3 * i + 1] = (int)((((r >> 20) & 0xFFFFF) * (uint64_t)(R + 1)) >> 20);
            out[3 * i + 2] = flip ? (int)(r >> 63) : 0;
        }
    } else { mi_record_host_error("mi_augment_plan", "mode is MI_AUG_FIXED, _CENTER or _RANDOM"); return -1; }
    return 0;
}
/* torchvision's RandomResizedCrop.get_params on a square image, drawn from the counter streams (include/resnet_mi.h).  Every product
 * and sum is rounded on its own (the file is compiled with contraction off), so math.log / exp / sqrt / round in Python give the same
 * integers (tests/rrcref.py). */
static double rrc_unit(uint64_t x) { return (double)(x >> 11) * 0x1p-53; }
static int rrc_clamp(long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }
int mi_augment_plan_rrc(int flip, uint64_t seed, int epoch, int64_t first_global_index, int n, int dim_in, double scale_lo, double scale_hi,
                        double ratio_lo, double ratio_hi, int *out) {
    if (n < 0 || dim_in < 1) { mi_record_host_error("mi_augment_plan_rrc", "need n >= 0 and dim_in >= 1"); return -1; }
    if (!(scale_lo > 0) || !(ratio_lo > 0) || !(scale_hi >= scale_lo) || !(ratio_hi >= ratio_lo)) {
        mi_record_host_error("mi_augment_plan_rrc", "need 0 < scale_lo <= scale_hi and 0 < ratio_lo <= ratio_hi"); return -1;
    }
    const uint64_t s = mi_splitmix64_at(seed, (uint64_t)(int64_t)epoch);
    const double area = (double)dim_in * (double)dim_in, log_lo = log(ratio_lo), log_hi = log(ratio_hi);
    for (int i = 0; i < n; i++) {
        const uint64_t k = mi_splitmix64_at(s, (uint64_t)(first_global_index + i));
        int h = 0, w = 0, row0 = 0, col0 = 0, t;
        for (t = 0; t < 10; t++) {
            const double target = area * (scale_lo + rrc_unit(mi_splitmix64_at(k, 4 * t)) * (scale_hi - scale_lo));
            const double ratio = exp(log_lo + rrc_unit(mi_splitmix64_at(k, 4 * t + 1)) * (log_hi - log_lo));
            const double fw = sqrt(target * ratio), fh = sqrt(target / ratio);
            if (!(fw >= 0.5 && fw <= dim_in + 0.5 && fh >= 0.5 && fh <= dim_in + 0.5)) continue; /* lrint of such a side is out of range */
            const long lw = lrint(fw), lh = lrint(fh); /* half to even */
            if (lw < 1 || lw > dim_in || lh < 1 || lh > dim_in) continue;
            w = (int)lw; h = (int)lh;
            row0 = (int)(((mi_splitmix64_at(k, 4 * t + 2) >> 32) * (uint64_t)(dim_in - h + 1)) >> 32);
            col0 = (int)(((mi_splitmix64_at(k, 4 * t + 3) >> 32) * (uint64_t)(dim_in - w + 1)) >> 32);
            break;
        }
        if (t == 10) { /* the fallback: the largest centred box of an allowed ratio */
            h = w = dim_in;
            if (ratio_lo > 1) h = rrc_clamp(lrint(dim_in / ratio_lo), 1, dim_in);
            else if (ratio_hi < 1) w = rrc_clamp(lrint(dim_in * ratio_hi), 1, dim_in);
            row0 = (dim_in - h) / 2; col0 = (dim_in - w) / 2;
        }
        out[5 * i] = row0; out[5 * i + 1] = col0; out[5 * i + 2] = h; out[5 * i + 3] = w;
        out[5 * i + 4] = flip ? (int)(mi_splitmix64_at(k, 40) >> 63) : 0;
    }
    return 0;
}
/* mixup / CutMix: what one step's batch is mixed with (include/resnet_mi.h, "mixing"; tests/mixref.py restates it with math.pow /
 * math.sqrt).  Every product, quotient and sum is rounded on its own, as in the RRC plan */
int mi_mix_plan(uint64_t seed, int epoch, int64_t step, int rank, int world, double mixup_alpha, double cutmix_alpha, double prob,
                double switch_prob, int dim, MiMixPlan *out) {
    const char *who = "mi_mix_plan";
    if (!out) { mi_record_host_error(who, "out is NULL"); return -1; }
    memset(out, 0, sizeof *out);
    out->lam = 1.f;
    if (!(mixup_alpha >= 0 && mixup_alpha <= 1) || !(cutmix_alpha >= 0 && cutmix_alpha <= 1)) {
        mi_record_host_error(who, "an alpha lies in (0, 1] (Johnk's method), or is 0: that mode is off"); return -1;
    }
    if (!(mixup_alpha > 0) && !(cutmix_alpha > 0)) { mi_record_host_error(who, "both alphas are 0: nothing to draw"); return -1; }
    if (!(prob >= 0 && prob <= 1) || !(switch_prob >= 0 && switch_prob <= 1)) { mi_record_host_error(who, "prob and switch_prob lie in [0, 1]"); return -1; }
    if (dim < 1 || dim > 16384) { mi_record_host_error(who, "need 1 <= dim <= 16384"); return -1; }
    if (world < 1 || rank < 0 || rank >= world) { mi_record_host_error(who, "need 0 <= rank < world"); return -1; }
    const uint64_t s = mi_splitmix64_at(seed, (uint64_t)(int64_t)epoch);
    const uint64_t k = mi_splitmix64_at(s, (uint64_t)step * (uint64_t)world + (uint64_t)rank); /* modulo 2^64: the trainer's first step is -1 */
    if (rrc_unit(mi_splitmix64_at(k, 0)) >= prob) return 0; /* mode 0 */
    const int cut_mode = mixup_alpha > 0 && cutmix_alpha > 0 ? rrc_unit(mi_splitmix64_at(k, 1)) < switch_prob : cutmix_alpha > 0;
    const double inv = 1.0 / (cut_mode ? cutmix_alpha : mixup_alpha);
    double lam = 0.5; /* no try taken */
    for (int t = 0; t < 64; t++) {
        const double X = pow(rrc_unit(mi_splitmix64_at(k, 2 + 2 * t)), inv), Y = pow(rrc_unit(mi_splitmix64_at(k, 3 + 2 * t)), inv);
        const double sum = X + Y;
        if (sum > 0 && sum <= 1) { lam = X / sum; break; }
    }
    out->mode = cut_mode ? 2 : 1;
    if (cut_mode) { /* timm's rand_bbox on a dim x dim image */
        const int D = dim, cut = (int)(D * sqrt(1.0 - lam));
        const int cy = (int)(((mi_splitmix64_at(k, 130) >> 32) * (uint64_t)D) >> 32), cx = (int)(((mi_splitmix64_at(k, 131) >> 32) * (uint64_t)D) >> 32);
        out->y0 = rrc_clamp(cy - cut / 2, 0, D); out->y1 = rrc_clamp(cy + cut / 2, 0, D);
        out->x0 = rrc_clamp(cx - cut / 2, 0, D); out->x1 = rrc_clamp(cx + cut / 2, 0, D);
        lam = 1.0 - (double)((int64_t)(out->y1 - out->y0) * (out->x1 - out->x0)) / (double)((int64_t)D * D);
    }
    out->lam = (float)lam;
    return 0;
}
/* random erasing: the boxes of one step's rows (include/resnet_mi.h, "random erasing"; tests/eraseref.py restates it with math.log / exp /
 * sqrt / round).  mi_erase_key: e of that text, the key of the rows' draws and the trainer's noise seed */
uint64_t mi_erase_key(uint64_t seed, int epoch, int64_t step, int rank, int world) {
    const uint64_t s = mi_splitmix64_at(seed, (uint64_t)(int64_t)epoch);
    const uint64_t k = mi_splitmix64_at(s, (uint64_t)step * (uint64_t)world + (uint64_t)rank); /* mi_mix_plan's step key */
    return mi_splitmix64_at(k, 1000);
}
int mi_erase_plan(uint64_t seed, int epoch, int64_t step, int rank, int world, int n, int dim, double prob, double scale_lo, double scale_hi,
                  double ratio_lo, double ratio_hi, int *out) {
    const char *who = "mi_erase_plan";
    if (n < 0 || (n > 0 && !out)) { mi_record_host_error(who, "need n >= 0 and out"); return -1; }
    if (dim < 1 || dim > 16384) { mi_record_host_error(who, "need 1 <= dim <= 16384"); return -1; }
    if (!(prob >= 0 && prob <= 1)) { mi_record_host_error(who, "prob lies in [0, 1]"); return -1; }
    if (!(scale_lo > 0) || !(ratio_lo > 0) || !(scale_hi >= scale_lo) || !(ratio_hi >= ratio_lo)) {
        mi_record_host_error(who, "need 0 < scale_lo <= scale_hi and 0 < ratio_lo <= ratio_hi"); return -1;
    }
    if (world < 1 || rank < 0 || rank >= world) { mi_record_host_error(who, "need 0 <= rank < world"); return -1; }
    const uint64_t e = mi_erase_key(seed, epoch, step, rank, world);
    const int D = dim;
    const double area = (double)D * (double)D, log_lo = log(ratio_lo), log_hi = log(ratio_hi);
    for (int i = 0; i < n; i++) {
        int *o = out + 4 * (size_t)i;
        o[0] = o[1] = o[2] = o[3] = 0;
        const uint64_t k = mi_splitmix64_at(e, (uint64_t)i);
        if (rrc_unit(mi_splitmix64_at(k, 0)) >= prob) continue;
        for (int t = 0; t < 10; t++) {
            const double target = area * (scale_lo + rrc_unit(mi_splitmix64_at(k, 1 + 4 * t)) * (scale_hi - scale_lo));
            const double ratio = exp(log_lo + rrc_unit(mi_splitmix64_at(k, 2 + 4 * t)) * (log_hi - log_lo));
            const double fh = sqrt(target * ratio), fw = sqrt(target / ratio);
            if (!(fh < D + 1.0 && fw < D + 1.0)) continue; /* rounds to D or more (or is no number): lrint stays in range below */
            const long lh = lrint(fh), lw = lrint(fw); /* half to even */
            if (!(lh < D && lw < D)) continue;
            o[2] = (int)lh; o[3] = (int)lw;
            o[0] = (int)(((mi_splitmix64_at(k, 3 + 4 * t) >> 32) * (uint64_t)(D - o[2] + 1)) >> 32);
            o[1] = (int)(((mi_splitmix64_at(k, 4 + 4 * t) >> 32) * (uint64_t)(D - o[3] + 1)) >> 32);
            break;
        }
    }
    return 0;
}
/* TrivialAugmentWide: the record of one (op, bin, sign) and the records of one step's rows (include/resnet_mi.h, "TrivialAugmentWide";
 * tests/taref.py restates it with Python's math and round).  The two tables are torch.linspace(0, 0.99, 31) and torch.linspace(0, 32, 31)
 * in float32, widened to double: torchvision's _augmentation_space(31) */
static const double ta_mag_099[MI_TA_BINS] = {
    0.0, 0.032999999821186066, 0.06599999964237213, 0.0989999994635582, 0.13199999928474426, 0.16499999165534973, 0.1979999989271164,
    0.23100000619888306, 0.2639999985694885, 0.296999990940094, 0.32999998331069946, 0.3630000054836273, 0.3959999978542328,
    0.42899999022483826, 0.4620000123977661, 0.4950000047683716, 0.527999997138977, 0.5609999895095825, 0.593999981880188,
    0.6270000338554382, 0.6600000262260437, 0.6930000185966492, 0.7260000109672546, 0.7590000033378601, 0.7919999957084656,
    0.824999988079071, 0.8580000400543213, 0.8910000324249268, 0.9240000247955322, 0.9570000171661377, 0.9900000095367432};
static const double ta_mag_32[MI_TA_BINS] = {
    0.0, 1.0666667222976685, 2.133333444595337, 3.200000286102295, 4.266666889190674, 5.333333492279053, 6.40000057220459,
    7.466667175292969, 8.533333778381348, 9.600000381469727, 10.666666984558105, 11.733333587646484, 12.80000114440918,
    13.866667747497559, 14.933334350585938, 15.999999046325684, 17.066665649414062, 18.133333206176758, 19.19999885559082,
    20.266666412353516, 21.333332061767578, 22.399999618530273, 23.46666717529297, 24.53333282470703, 25.600000381469727,
    26.66666603088379, 27.733333587646484, 28.799999237060547, 29.866666793823242, 30.933332443237305, 32.0};
static const double TA_PI = 3.141592653589793;
static int ta_fix(double v) { return (int)floor(v * 65536.0 + 0.5); } /* Pillow's FIX */
/* Python's round(v, 15) for |v| <= 1: the exact value rounded half to even at 15 decimal places, then the nearest double */
static double ta_round15(double v) {
    char buf[40];
    snprintf(buf, sizeof buf, "%.15f", v);
    return strtod(buf, NULL);
}
static void ta_fixed(const double a[6], int A[6]) {
    A[0] = ta_fix(a[0]); A[1] = ta_fix(a[1]); A[2] = ta_fix(a[2] + a[0] * 0.5 + a[1] * 0.5);
    A[3] = ta_fix(a[3]); A[4] = ta_fix(a[4]); A[5] = ta_fix(a[5] + a[3] * 0.5 + a[4] * 0.5);
}
int mi_ta_row(int op, int bin, int neg, int dim, MiTaRow *out) {
    const char *who = "mi_ta_row";
    if (!out) { mi_record_host_error(who, "out is NULL"); return -1; }
    if (op < 0 || op >= MI_TA_OPS) { mi_record_host_error(who, "op lies in [0, 14)"); return -1; }
    if (bin < 0 || bin >= MI_TA_BINS) { mi_record_host_error(who, "bin lies in [0, 31)"); return -1; }
    if (neg != 0 && neg != 1) { mi_record_host_error(who, "neg is 0 or 1"); return -1; }
    if (dim < 1 || dim > 4096) { mi_record_host_error(who, "need 1 <= dim <= 4096"); return -1; }
    const int is_signed = op >= MI_TA_SHEAR_X && op <= MI_TA_SHARPNESS;
    double m = 0;
    switch (op) {
    case MI_TA_SHEAR_X: case MI_TA_SHEAR_Y: case MI_TA_BRIGHTNESS: case MI_TA_COLOR: case MI_TA_CONTRAST: case MI_TA_SHARPNESS: m = ta_mag_099[bin]; break;
    case MI_TA_TRANSLATE_X: case MI_TA_TRANSLATE_Y: m = ta_mag_32[bin]; break;
    case MI_TA_ROTATE: m = 4.5 * bin; break;
    case MI_TA_POSTERIZE: m = 8 - (bin * 2 + 5) / 10; break; /* round(bin / 5): bin / 5 is never half an integer */
    case MI_TA_SOLARIZE: m = 255.0 - 8.5 * bin; break;
    default: break;
    }
    memset(out, 0, sizeof *out);
    out->op = op; out->bin = bin; out->neg = is_signed ? neg : 0;
    if (out->neg) m = -m;
    out->magnitude = m;
    double a[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    switch (op) {
    case MI_TA_BRIGHTNESS: case MI_TA_COLOR: case MI_TA_CONTRAST: case MI_TA_SHARPNESS: out->factor = (float)(1.0 + m); break;
    case MI_TA_POSTERIZE: out->arg = ~((1 << (8 - (int)m)) - 1) & 255; break;
    case MI_TA_SOLARIZE: out->arg = (int)ceil(m); break;
    case MI_TA_SHEAR_X: case MI_TA_SHEAR_Y: {
        const double deg = atan(m) * (180.0 / TA_PI);   /* math.degrees */
        const double t = tan(deg * (TA_PI / 180.0));    /* math.radians */
        a[op == MI_TA_SHEAR_X ? 1 : 3] = t;
        ta_fixed(a, out->A);
        break;
    }
    case MI_TA_TRANSLATE_X: a[2] = -(double)(int)m; ta_fixed(a, out->A); break;
    case MI_TA_TRANSLATE_Y: a[5] = -(double)(int)m; ta_fixed(a, out->A); break;
    case MI_TA_ROTATE: {
        double mod = fmod(m, 360.0); /* Python's %: the sign of the divisor */
        if (mod != 0) { if (mod < 0) mod += 360.0; } else mod = 0.0;
        const double r = -(mod * (TA_PI / 180.0)), c = dim / 2.0;
        a[0] = ta_round15(cos(r)); a[1] = ta_round15(sin(r)); a[3] = ta_round15(-sin(r)); a[4] = ta_round15(cos(r));
        a[2] = a[0] * -c + a[1] * -c + 0.0; a[2] += c;
        a[5] = a[3] * -c + a[4] * -c + 0.0; a[5] += c;
        ta_fixed(a, out->A);
        break;
    }
    default: break;
    }
    return 0;
}
int mi_ta_plan(uint64_t seed, int epoch, int64_t step, int rank, int world, int n, int dim, MiTaRow *out) {
    const char *who = "mi_ta_plan";
    if (n < 0 || (n > 0 && !out)) { mi_record_host_error(who, "need n >= 0 and out"); return -1; }
    if (dim < 1 || dim > 4096) { mi_record_host_error(who, "need 1 <= dim <= 4096"); return -1; }
    if (world < 1 || rank < 0 || rank >= world) { mi_record_host_error(who, "need 0 <= rank < world"); return -1; }
    const uint64_t s = mi_splitmix64_at(seed, (uint64_t)(int64_t)epoch);
    const uint64_t k = mi_splitmix64_at(s, (uint64_t)step * (uint64_t)world + (uint64_t)rank); /* mi_mix_plan's step key */
    const uint64_t a = mi_splitmix64_at(k, 2000);
    for (int i = 0; i < n; i++) {
        const uint64_t ki = mi_splitmix64_at(a, (uint64_t)i);
        const int op = (int)(((mi_splitmix64_at(ki, 0) >> 32) * (uint64_t)MI_TA_OPS) >> 32);
        const int bin = (int)(((mi_splitmix64_at(ki, 1) >> 32) * (uint64_t)MI_TA_BINS) >> 32);
        if (mi_ta_row(op, bin, (int)(mi_splitmix64_at(ki, 2) >> 63), dim, out + i)) return -1;
    }
    return 0;
}
/* double-buffered H2D: while step t runs, batch t+1 of the resident shard goes pinned -> device on the copy stream
 * (the reference copies synchronously at the top of every step, resnet.cu:1315-1316) */
void mi_batch_set_prefetch(Batch *b, int on) {
    BatchExt *e = mi_batch_ext(b);
    e->prefetch = on; e->have_next = 0;
    const size_t bytes = (size_t)b->n_images * b->image_size * sizeof(float);
    if (on && !e->images_next) {
        e->images_next = (float *)mid_malloc(bytes);
        e->labels_next = (int *)mid_malloc((size_t)b->n_images * sizeof(int));
        e->labels_next_host = (int *)mid_malloc_host((size_t)b->n_images * sizeof(int));
        e->ev_next = mid_event_create();
        e->ev_compute = mid_event_create();
    }
    if (on && e->source == MI_SRC_SHARDS_U8) u8_ensure(b, e); /* bytes are staged, not floats */
    else if (on && !e->pinned_next) {
        e->stage_next = (float *)mid_malloc(bytes);
        e->pinned_next = (float *)mid_malloc_host(bytes);
    }
}
/* enqueue batch (shard resident in host RAM, index bi) on the copy stream into the *_next buffers */
static void prefetch_enqueue(Batch *b, BatchExt *e, int bi) {
    MiGlobal *g = mi_global();
    const int N = b->n_images;
    const size_t px = (size_t)N * b->image_size, bytes = px * sizeof(float);
    memcpy(e->pinned_next, b->full_shard_images + (size_t)bi * px, bytes);
    memcpy(e->labels_next_host, b->full_shard_correct_classes + (size_t)bi * N, (size_t)N * sizeof(int));
    /* images_next / labels_next were the PREVIOUS step's batch until the swap a moment ago: that step's backward (stem weight
     * gradient) and update_parameters' input_reset memsets may still be queued on the compute stream against them, and
     * update_parameters no longer synchronises the host.  The copy stream therefore waits for everything the compute stream
     * holds right now before it overwrites the buffers (an event, not a host sync: the caller goes on queueing). */
    mid_event_record(e->ev_compute, g->compute);
    mid_stream_wait_event(g->copy, e->ev_compute);
    if (e->layout == MI_LAYOUT_NHWC) {
        mid_memcpy_h2d(e->stage_next, e->pinned_next, bytes, g->copy);
        mid_nhwc_to_nchw(g->copy, e->stage_next, e->images_next, N, b->image_dim, b->image_dim, b->image_size / (b->image_dim * b->image_dim));
    } else mid_memcpy_h2d(e->images_next, e->pinned_next, bytes, g->copy);
    mid_memcpy_h2d(e->labels_next, e->labels_next_host, (size_t)N * sizeof(int), g->copy);
    mid_event_record(e->ev_next, g->copy);
    e->have_next = 1; e->next_shard_id = b->cur_shard_id; e->next_batch_in_shard = bi;
}
/* MI_SRC_SHARDS_U8: batch bi of the resident shard -> pinned set k -> device on stream s, decoded into `images`; the plan is in
 * plan_pinned[k] already */
static void u8_enqueue(Batch *b, BatchExt *e, int bi, int k, mid_stream s, float *images, int *labels_dev, int *labels_host) {
    const int N = b->n_images;
    const size_t bytes = (size_t)N * e->u8_dim_in * e->u8_dim_in * 3;
    memcpy(e->u8_pinned[k], e->u8_shard + (size_t)bi * bytes, bytes);
    memcpy(labels_host, b->full_shard_correct_classes + (size_t)bi * N, (size_t)N * sizeof(int));
    mid_memcpy_h2d(e->u8_dev[k], e->u8_pinned[k], bytes, s);
    mid_memcpy_h2d(labels_dev, labels_host, (size_t)N * sizeof(int), s);
    const int rrc = e->aug_mode == MI_AUG_RRC;
    mid_memcpy_h2d(e->plan_dev[k], e->plan_pinned[k], (size_t)N * (rrc ? 5 : 3) * sizeof(int), s);
    if (rrc && e->rrc_antialias) mid_resample_aa_u8(s, e->u8_dev[k], e->plan_dev[k], images, N, e->u8_dim_in, b->image_dim, b->image_dim, 0, 0);
    else if (rrc) mid_resample_u8(s, e->u8_dev[k], e->plan_dev[k], images, N, e->u8_dim_in, b->image_dim);
    else mid_decode_u8(s, e->u8_dev[k], e->plan_dev[k], images, N, e->u8_dim_in, b->image_dim);
}
/* the plan of this rank's batch bi of the resident shard at `epoch` into plan_pinned[k]; 0, or -1 with a message */
static int u8_plan(Batch *b, BatchExt *e, int bi, int epoch, int k) {
    const int N = b->n_images;
    if (e->aug_mode == MI_AUG_FIXED && !e->u8_have_crops) {
        fprintf(stderr, "resnet_mi: MI_AUG_FIXED needs %s/%03d.crops\n", e->shard_dir, b->cur_shard_id);
        return -1;
    }
    const int64_t first = (int64_t)b->cur_shard_id * b->shard_n_images + (int64_t)bi * N;
    if (e->aug_mode == MI_AUG_RRC ? mi_augment_plan_rrc(e->aug_flip, e->aug_seed, epoch, first, N, e->u8_dim_in, e->rrc_scale[0], e->rrc_scale[1],
                                                       e->rrc_ratio[0], e->rrc_ratio[1], e->plan_pinned[k]) :
        mi_augment_plan(e->aug_mode, e->aug_flip, e->aug_seed, epoch, first, N, e->u8_dim_in, b->image_dim,
                        e->u8_have_crops ? e->u8_crops + (size_t)bi * N * 2 : NULL, e->plan_pinned[k])) {
        fprintf(stderr, "resnet_mi: no augmentation plan for shard %d batch %d: %s\n", b->cur_shard_id, bi, mi_last_error());
        return -1;
    }
    return 0;
}
void mi_batch_source_buffer(Batch *b, const char *images_path, const char *labels_path, int layout) {
    BatchExt *e = mi_batch_ext(b);
    e->source = MI_SRC_BUFFER; e->layout = layout; set_str(&e->images_path, images_path); set_str(&e->labels_path, labels_path);
    e->pool_next = 0; /* "not read yet" */
}
void mi_batch_source_host(Batch *b, int layout) {
    BatchExt *e = mi_batch_ext(b);
    e->source = MI_SRC_HOST; e->layout = layout;
}
/* data parallel: global batch g of a shard = images [g*world*N, (g+1)*world*N); rank r reads the r-th N of it.  Every rank
 * advances cur_batch_in_shard by one per step and rolls to the next shard at the same step. */
void mi_batch_set_rank_slice(Batch *b, int rank, int world) {
    BatchExt *e = mi_batch_ext(b);
    if (world < 1) world = 1;
    if (rank < 0 || rank >= world) rank = 0;
    e->rank = rank; e->world = world; e->have_next = 0;
}
int mi_batch_last_status(const Batch *b) { return mi_batch_ext((Batch *)b)->status; }

/* Synthetic pool: batch j of the pool = stream elements [j*n, (j+1)*n) of the two seeds, generated on the
 * device (NCHW order) and kept in HBM; load_new_batch cycles through it with a D2D copy. */
void mi_batch_source_synthetic(Batch *b, uint64_t seed_images, uint64_t seed_labels, int n_classes, int pool_batches) {
    BatchExt *e = mi_batch_ext(b);
    MiGlobal *g = mi_global();
    if (pool_batches < 1) pool_batches = 1;
    e->source = MI_SRC_SYNTHETIC; e->layout = MI_LAYOUT_NCHW;
    e->seed_images = seed_images; e->seed_labels = seed_labels; e->n_classes = n_classes;
    mid_free(e->pool_images); mid_free(e->pool_labels); free(e->pool_labels_host);
    const size_t per = (size_t)b->n_images * b->image_size;
    e->pool_batches = pool_batches; e->pool_next = 0;
    e->pool_images = (float *)mid_malloc(per * pool_batches * sizeof(float));
    e->pool_labels = (int *)mid_malloc((size_t)b->n_images * pool_batches * sizeof(int));
    e->pool_labels_host = (int *)malloc((size_t)b->n_images * pool_batches * sizeof(int));
    mid_fill_uniform(g->compute, e->pool_images, per * pool_batches, seed_images, 0, -124.0f, 152.0f);
    mi_synth_labels(e->pool_labels_host, (size_t)b->n_images * pool_batches, seed_labels, 0, n_classes);
    mid_memcpy_h2d(e->pool_labels, e->pool_labels_host, (size_t)b->n_images * pool_batches * sizeof(int), g->compute);
    mid_stream_sync(g->compute);
}

static size_t read_file(const char *path, void *dst, size_t elem, size_t count) {
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    const size_t n = fread(dst, elem, count, f);
    fclose(f);
    return n;
}

static void upload(Batch *b, BatchExt *e) {
    MiGlobal *g = mi_global();
    const size_t bytes = (size_t)b->n_images * b->image_size * sizeof(float);
    if (e->layout == MI_LAYOUT_NHWC) {
        if (!e->stage_dev) e->stage_dev = (float *)mid_malloc(bytes);
        mid_memcpy_h2d(e->stage_dev, b->images_float_cpu, bytes, g->compute);
        mid_nhwc_to_nchw(g->compute, e->stage_dev, b->images, b->n_images, b->image_dim, b->image_dim,
                         b->image_size / (b->image_dim * b->image_dim));
    } else {
        mid_memcpy_h2d(b->images, b->images_float_cpu, bytes, g->compute);
    }
    mid_memcpy_h2d(b->correct_classes, b->correct_classes_cpu, (size_t)b->n_images * sizeof(int), g->compute);
    mid_stream_sync(g->compute); /* the reference's cudaMemcpy is blocking (:1315-1316) */
}

/* resnet.cu:1235-1325 */
void load_new_batch(Train_ResNet *trainer, Class_Metadata *class_metadata, Batch *b) {
    (void)class_metadata;
    mi_trainer_poll_errors(trainer); /* check_errors of the step that just ended, while its batch and activations are still there */
    BatchExt *e = mi_batch_ext(b);
    MiGlobal *g = mi_global();
    const int N = b->n_images;
    const size_t total_pixels = (size_t)N * b->image_size;
    e->status = 0;
    if (e->source == MI_SRC_SHARDS) {
        const int W = e->world, R = e->rank;
        /* later variants skip a ragged tail instead of assuming divisibility (resnet_cudnn_lowmem.cu:1293-1297) */
        if (trainer->init_loaded || b->cur_shard_id == -1 || (b->cur_batch_in_shard + 1) * W * N > b->shard_n_images) {
            if (!trainer->init_loaded) b->cur_shard_id += 1;
            if (!b->full_shard_images) {
                b->full_shard_images = (float *)malloc((size_t)b->shard_n_images * b->image_size * sizeof(float));
                b->full_shard_correct_classes = (int *)malloc((size_t)b->shard_n_images * sizeof(int));
            }
            char *pi = NULL, *pl = NULL;
            if (asprintf(&pi, "%s/%03d.images", e->shard_dir, b->cur_shard_id) < 0 || asprintf(&pl, "%s/%03d.labels", e->shard_dir, b->cur_shard_id) < 0) exit(1);
            const size_t ni = read_file(pi, b->full_shard_images, sizeof(float), (size_t)b->shard_n_images * b->image_size);
            const size_t nl = read_file(pl, b->full_shard_correct_classes, sizeof(int), b->shard_n_images);
            if (ni != (size_t)b->shard_n_images * b->image_size || nl != (size_t)b->shard_n_images) {
                fprintf(stderr, "resnet_mi: cannot read shard %s (%zu of %zu floats)\n", pi, ni, (size_t)b->shard_n_images * b->image_size);
                e->status = -1;
            }
            free(pi); free(pl);
            if (!trainer->init_loaded) b->cur_batch_in_shard = 0;
            trainer->init_loaded = 0;
        }
        if (e->status == 0) {
            const int bi = b->cur_batch_in_shard * W + R; /* this rank's batch of the shard */
            if (e->prefetch && e->have_next && e->next_shard_id == b->cur_shard_id && e->next_batch_in_shard == bi) {
                /* batch already on the device: order the compute stream after the copy and swap buffers */
                mid_stream_wait_event(g->compute, e->ev_next);
                mid_event_sync(e->ev_next); /* the pinned staging buffer is rewritten below */
                float *ti = b->images; b->images = e->images_next; e->images_next = ti;
                int *tl = b->correct_classes; b->correct_classes = e->labels_next; e->labels_next = tl;
                memcpy(b->correct_classes_cpu, e->labels_next_host, (size_t)N * sizeof(int));
                e->have_next = 0;
            } else {
                memcpy(b->images_float_cpu, b->full_shard_images + (size_t)bi * total_pixels, total_pixels * sizeof(float));
                memcpy(b->correct_classes_cpu, b->full_shard_correct_classes + (size_t)bi * N, (size_t)N * sizeof(int));
                upload(b, e);
            }
            if (e->prefetch && (b->cur_batch_in_shard + 2) * W * N <= b->shard_n_images) {
                /* the swapped-out buffer may still be read (stem weight gradient) and cleared (input_reset) by the step that
                 * just ended: prefetch_enqueue orders the copy stream behind the compute stream before writing into it */
                prefetch_enqueue(b, e, (b->cur_batch_in_shard + 1) * W + R);
            }
        }
    } else if (e->source == MI_SRC_SHARDS_U8) {
        /* rotation, ragged tail, rank slices and bookkeeping as MI_SRC_SHARDS above */
        const int W = e->world, R = e->rank, epoch = trainer->cur_epoch;
        const size_t img_bytes = (size_t)e->u8_dim_in * e->u8_dim_in * 3;
        if (trainer->init_loaded || b->cur_shard_id == -1 || (b->cur_batch_in_shard + 1) * W * N > b->shard_n_images) {
            if (!trainer->init_loaded) b->cur_shard_id += 1;
            if (!e->u8_shard) {
                e->u8_shard = (uint8_t *)malloc((size_t)b->shard_n_images * img_bytes);
                e->u8_crops = (int *)malloc((size_t)b->shard_n_images * 2 * sizeof(int));
            }
            if (!b->full_shard_correct_classes) b->full_shard_correct_classes = (int *)malloc((size_t)b->shard_n_images * sizeof(int));
            char *pi = NULL, *pl = NULL, *pc = NULL;
            if (asprintf(&pi, "%s/%03d.images_u8", e->shard_dir, b->cur_shard_id) < 0 || asprintf(&pl, "%s/%03d.labels", e->shard_dir, b->cur_shard_id) < 0 ||
                asprintf(&pc, "%s/%03d.crops", e->shard_dir, b->cur_shard_id) < 0) exit(1);
            const size_t ni = read_file(pi, e->u8_shard, 1, (size_t)b->shard_n_images * img_bytes);
            const size_t nl = read_file(pl, b->full_shard_correct_classes, sizeof(int), b->shard_n_images);
            e->u8_have_crops = read_file(pc, e->u8_crops, sizeof(int), (size_t)b->shard_n_images * 2) == (size_t)b->shard_n_images * 2;
            if (ni != (size_t)b->shard_n_images * img_bytes || nl != (size_t)b->shard_n_images) {
                fprintf(stderr, "resnet_mi: cannot read shard %s (%zu of %zu bytes)\n", pi, ni, (size_t)b->shard_n_images * img_bytes);
                e->status = -1;
            }
            free(pi); free(pl); free(pc);
            e->have_next = 0; /* cut from the shard this one replaced */
            if (!trainer->init_loaded) b->cur_batch_in_shard = 0;
            trainer->init_loaded = 0;
        }
        if (e->status == 0) {
            const int bi = b->cur_batch_in_shard * W + R; /* this rank's batch of the shard */
            u8_ensure(b, e);
            /* the draw changes with the epoch and mi_trainer_end_epoch rewinds to shard 0: a prefetched batch counts only for its epoch */
            if (e->prefetch && e->have_next && e->next_shard_id == b->cur_shard_id && e->next_batch_in_shard == bi && e->next_epoch == epoch) {
                mid_stream_wait_event(g->compute, e->ev_next);
                mid_event_sync(e->ev_next); /* the pinned staging buffers are rewritten below */
                float *ti = b->images; b->images = e->images_next; e->images_next = ti;
                int *tl = b->correct_classes; b->correct_classes = e->labels_next; e->labels_next = tl;
                memcpy(b->correct_classes_cpu, e->labels_next_host, (size_t)N * sizeof(int));
                memcpy(e->plan_pinned[0], e->plan_pinned[1], (size_t)N * 5 * sizeof(int));
                e->have_next = 0; e->have_plan = 1;
            } else if (u8_plan(b, e, bi, epoch, 0) == 0) {
                u8_enqueue(b, e, bi, 0, g->compute, b->images, b->correct_classes, b->correct_classes_cpu);
                mid_stream_sync(g->compute); /* blocking, as the fp32 sources: the pinned buffers are free again */
                e->have_plan = 1;
            } else e->status = -1;
            if (e->status == 0 && e->prefetch && (b->cur_batch_in_shard + 2) * W * N <= b->shard_n_images) {
                const int nb = (b->cur_batch_in_shard + 1) * W + R;
                if (e->have_next) { mid_event_sync(e->ev_next); e->have_next = 0; } /* a prefetch nobody took still reads the pinned set */
                if (u8_plan(b, e, nb, epoch, 1) == 0) {
                    /* the copy stream waits for what the compute stream holds against images_next / labels_next (see prefetch_enqueue) */
                    mid_event_record(e->ev_compute, g->compute);
                    mid_stream_wait_event(g->copy, e->ev_compute);
                    u8_enqueue(b, e, nb, 1, g->copy, e->images_next, e->labels_next, e->labels_next_host);
                    mid_event_record(e->ev_next, g->copy);
                    e->have_next = 1; e->next_shard_id = b->cur_shard_id; e->next_batch_in_shard = nb; e->next_epoch = epoch;
                }
            }
        }
    } else if (e->source == MI_SRC_BUFFER) {
        if (!e->pool_next) {
            const size_t ni = read_file(e->images_path, b->images_float_cpu, sizeof(float), total_pixels);
            const size_t nl = read_file(e->labels_path, b->correct_classes_cpu, sizeof(int), N);
            if (ni != total_pixels || nl != (size_t)N) { fprintf(stderr, "resnet_mi: cannot read %s / %s\n", e->images_path, e->labels_path); e->status = -1; }
            e->pool_next = 1;
        }
        if (e->status == 0) upload(b, e);
    } else if (e->source == MI_SRC_HOST) {
        upload(b, e);
    } else { /* synthetic, resident in HBM */
        const int j = e->pool_next;
        mid_memcpy_d2d(b->images, e->pool_images + (size_t)j * total_pixels, total_pixels * sizeof(float), g->compute);
        mid_memcpy_d2d(b->correct_classes, e->pool_labels + (size_t)j * N, (size_t)N * sizeof(int), g->compute);
        memcpy(b->correct_classes_cpu, e->pool_labels_host + (size_t)j * N, (size_t)N * sizeof(int));
        e->pool_next = (j + 1) % e->pool_batches;
    }
    /* TrivialAugmentWide, random erasing, then mixup / CutMix (the per-sample transforms in front of the collate step), every source:
     * behind the load (or the prefetch swap) on the compute stream, drawn at the step the dump saves */
    if (e->status == 0) mi_trainer_ta_batch(trainer, b, e->rank, e->world);
    if (e->status == 0) mi_trainer_erase_batch(trainer, b, e->rank, e->world);
    if (e->status == 0) mi_trainer_mix_batch(trainer, b, e->rank, e->world);
    b->cur_batch_in_shard += 1;
    trainer->cur_dump_id += 1;
}

/* resnet.cu:1331-1381 */
static void text_file_to_buffer(void *buffer, const char *filename, int as_int) {
    FILE *fp = fopen(filename, "r");
    if (!fp) exit(EXIT_FAILURE); /* resnet.cu:1341-1342 */
    char *line = NULL;
    size_t len = 0;
    int cnt = 0;
    while (getline(&line, &len, fp) != -1) {
        if (as_int) ((int *)buffer)[cnt] = atoi(line);
        else ((char **)buffer)[cnt] = strdup(line);
        cnt++;
    }
    fclose(fp);
    free(line);
}
Class_Metadata *populate_class_info(char *label_filename, char *synset_filename, char *class_size_filename, int n_classes) {
    Class_Metadata *c = (Class_Metadata *)malloc(sizeof(Class_Metadata));
    c->labels = (char **)calloc(n_classes, sizeof(char *));
    c->synsets = (char **)calloc(n_classes, sizeof(char *));
    c->counts = (int *)calloc(n_classes, sizeof(int));
    text_file_to_buffer(c->labels, label_filename, 0);
    text_file_to_buffer(c->synsets, synset_filename, 0);
    text_file_to_buffer(c->counts, class_size_filename, 1);
    c->n_classes = n_classes;
    return c;
}
