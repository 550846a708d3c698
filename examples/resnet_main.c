/*
 * resnet_main.c -- the reference's driver (main() of resnet.cu:3222-3429) rebuilt on libresnet_mi.so: same call
 * sequence, same per-iteration printout (resnet.cu:3386) and avg_loss_log.txt (resnet.cu:3388), with the literals of
 * resnet.cu:3245-3299 exposed as command-line options and the data source selectable (the reference hard-codes
 * /mnt/storage paths).  Host loss/accuracy loop copied in spirit from resnet.cu:3363-3383 (it is the caller's code).
 *
 *   gcc -O2 -Iinclude examples/resnet_main.c -Lresnet_amd -lresnet_mi -lm -Wl,-rpath,$PWD/resnet_amd -o ResNetMI
 *   ./ResNetMI --iters 20 --batch 64                       synthetic data, reference-defined ResNet-50
 *   ./ResNetMI --shards /data/train_data_shards/nchw --layout nchw --shard-images 32768 --batch 256
 *   ./ResNetMI --shards-u8 /data/train_data_shards/u8 --dim-in 256 --augment random --aug-seed 7 --shard-images 32768 --batch 256
 *              uint8 shards of whole 256^2 images (tools/build_shards --u8): crop, flip and float conversion on the device, a new
 *              draw per epoch; --augment fixed (default: the shard's own crops, the reference's pixels) | center | random | rrc, --no-flip
 *   ./ResNetMI --shards-u8 /data/train_data_shards/u8 --augment rrc --rrc-scale 0.08,1 --rrc-ratio 0.75,1.3333333333333333 --batch 256
 *              random-resized crop: a box of LO .. HI of the image's area and of aspect ratio LO .. HI (the defaults shown), resampled
 *              to the input size on the device; --rrc-antialias: scaled as Pillow's BILINEAR scales bytes (the filter widened by the
 *              scale factor, mi_batch_set_antialias), not by the two-tap gather
 *   ./ResNetMI --label-smoothing 0.1 --topk 5 --device-loss
 *              the loss head on the device (mi_trainer_set_loss): label-smoothed cross entropy, loss and top-1 / top-K error counted
 *              there, one line of totals per epoch; --device-loss also drops forward_pass's blocking copy of the predictions
 *   ./ResNetMI --label-smoothing 0.1 --mixup 0.2 --cutmix 1.0 --mix-prob 1.0 --mix-seed 7
 *              mixup / CutMix on the device at every load (mi_trainer_set_mix; implies the device loss head): Beta(A, A) weights with A in
 *              (0, 1], 0 = that mode off; with both on each step draws one of them with equal odds; --mix-prob P: the share of steps mixed
 *   ./ResNetMI --random-erase 0.1 --erase-mode noise --erase-seed 7
 *              random erasing on the device at every load, in front of the mix step (mi_trainer_set_erase): with probability P a row gets
 *              one box of 0.02 .. 0.33 of its area, aspect 0.3 .. 3.3 (torchvision's --random-erase), filled with the mean pixel (the
 *              default, --erase-mode const) or with noise of ImageNet's per-channel deviation around it (timm's pixel mode)
 *   ./ResNetMI --auto-augment ta_wide --ta-seed 7
 *              TrivialAugmentWide on the device at every load, in front of erasing and mixing (mi_trainer_set_trivial_augment): per row one of
 *              14 Pillow operations at one of 31 strengths, Pillow's bytes bit for bit (torchvision's --auto-augment ta_wide)
 *   ./ResNetMI --bn-momentum 0.1 --val-u8 /data/val_shards/u8 --val-dim-in 256 --val-every 5000
 *              evaluation: running statistics of every batch norm (mi_trainer_track_running_stats; --val-u8 alone implies momentum 0.1) and,
 *              every STEPS iterations and at the end of every epoch, the eval pass over every %03d.images_u8 / %03d.labels under DIR
 *              (whole dim-in^2 images, centre crop): loss per image, top-1 and top-K error of the set; --val-resize N: every image is
 *              first scaled to N x N (antialiased, as Pillow) and the centre crop is taken from that: torchvision's --val-resize-size
 *   ./ResNetMI --ema 0.99998 --ema-every 32 --ema-warmup --val-u8 /data/val_shards/u8
 *              weight averaging (mi_trainer_set_ema): an exponential moving average of the parameters and the batch-norm running statistics,
 *              updated on the device behind every N-th update_parameters (default 1) with e <- e + (1 - DECAY) (p - e); --ema-warmup: timm's
 *              min(DECAY, (1 + k) / (10 + k)) for update k.  DECAY is used as given: torchvision's correction for world, batch, N and the
 *              number of epochs is the caller's.  --ema alone implies --bn-momentum 0.1; with --val-u8 every validation is printed twice,
 *              for the raw weights and for the EMA weights
 *   ./ResNetMI --batch 256 --accum 16 --accum-scale 0.0625
 *              gradient accumulation (mi_trainer_set_accumulation): one optimizer update per K iterations on the sum of their gradients
 *              times S (default 1: the sum, what a batch K times as large would give; 1/K: the mean over the micro-batches).  An
 *              iteration stays one micro-batch: the printout, --iters and --val-every count micro-batches, --ema-every counts updates
 *   ./ResNetMI --optimizer sgd --momentum 0.9 --lr 0.5 --wd 0.00002 --norm-weight-decay 0 --clip-grad-norm 256
 *              --optimizer adam (default) | sgd | lars (mi_trainer_set_optimizer; --momentum M, default 0.9).  --norm-weight-decay X (sgd):
 *              BN gamma / beta decay with X in place of --wd (torchvision's flag).  --clip-grad-norm X: every applied update first scales
 *              the gradient so that its global L2 norm is at most X (mi_trainer_set_clip_grad_norm), on the device; the gradient is a batch
 *              SUM (times --accum-scale under --accum), so X is torchvision's value times the batch size.  Each epoch then ends with a
 *              line of its clipped / total updates and the last gradient norm
 *   ./ResNetMI --labels-file id_to_label_mapping.txt --synsets-file id_to_synset_mapping.txt --counts-file id_to_img_count_mapping.txt
 *              the class metadata of resnet.cu:3236-3242: iterations per epoch = ceil(sum of the class counts / batch) (:3309)
 *              unless --iters says otherwise
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "resnet_mi.h"

static const char *opt(int argc, char **argv, const char *name, const char *def) {
    for (int i = 1; i + 1 < argc; i++) if (!strcmp(argv[i], name)) return argv[i + 1];
    return def;
}

/* the whole validation set, shard by shard through mi_trainer_eval_u8 (resize > 0: mi_trainer_eval_u8_resized; each call returns its own
 * total); 0, or -1 with a message printed */
static int validate_one(Train_ResNet *trainer, const char *dir, int dim_in, int resize, int topk, const char *when) {
    MiLossMetrics sum = {0};
    const size_t img = (size_t)dim_in * dim_in * 3;
    for (int id = 0;; id++) {
        char path[4096];
        snprintf(path, sizeof path, "%s/%03d.labels", dir, id);
        FILE *fl = fopen(path, "rb");
        if (!fl) break;
        fseek(fl, 0, SEEK_END);
        const long n = ftell(fl) / (long)sizeof(int);
        fseek(fl, 0, SEEK_SET);
        snprintf(path, sizeof path, "%s/%03d.images_u8", dir, id);
        FILE *fi = fopen(path, "rb");
        int *labels = (int *)malloc((size_t)(n > 0 ? n : 1) * sizeof(int));
        uint8_t *images = (uint8_t *)malloc((size_t)(n > 0 ? n : 1) * img);
        MiLossMetrics m = {0};
        int ok = fi && n > 0 && labels && images && fread(labels, sizeof(int), (size_t)n, fl) == (size_t)n &&
                 fread(images, img, (size_t)n, fi) == (size_t)n;
        if (!ok) fprintf(stderr, "validation shard %03d under %s is missing, empty or short\n", id, dir);
        else if (resize > 0 ? mi_trainer_eval_u8_resized(trainer, images, labels, n, dim_in, resize, topk, &m)
                            : mi_trainer_eval_u8(trainer, images, labels, n, dim_in, topk, &m)) { fprintf(stderr, "%s\n", mi_last_error()); ok = 0; }
        fclose(fl);
        if (fi) fclose(fi);
        free(labels); free(images);
        if (!ok) return -1;
        sum.loss_sum += m.loss_sum; sum.rows += m.rows; sum.wrong_top1 += m.wrong_top1; sum.wrong_topk += m.wrong_topk; sum.batches += m.batches;
    }
    if (!sum.rows) { fprintf(stderr, "no %%03d.images_u8 / %%03d.labels under %s\n", dir); return -1; }
    printf("Validation (%s) ----- Images: %lld, Avg. Loss: %.4f, Top-1 error: %.2f%%, Top-%d error: %.2f%%\n", when, (long long)sum.rows,
           sum.loss_sum / (double)sum.rows, 100.0 * (double)sum.wrong_top1 / (double)sum.rows, topk, 100.0 * (double)sum.wrong_topk / (double)sum.rows);
    return 0;
}
/* with --ema: the set twice, scored with the raw weights and with the averaged ones (mi_trainer_eval_use_ema) */
static int validate(Train_ResNet *trainer, const char *dir, int dim_in, int resize, int topk, const char *when, int ema) {
    char label[64];
    if (!ema) return validate_one(trainer, dir, dim_in, resize, topk, when);
    snprintf(label, sizeof label, "%s, raw weights", when);
    if (validate_one(trainer, dir, dim_in, resize, topk, label)) return -1;
    snprintf(label, sizeof label, "%s, EMA weights", when);
    if (mi_trainer_eval_use_ema(trainer, 1)) { fprintf(stderr, "%s\n", mi_last_error()); return -1; }
    const int rc = validate_one(trainer, dir, dim_in, resize, topk, label);
    mi_trainer_eval_use_ema(trainer, 0);
    return rc;
}

int main(int argc, char **argv) {
    const int N_CLASSES = atoi(opt(argc, argv, "--classes", "1000"));
    const int INPUT_DIM = atoi(opt(argc, argv, "--input", "224"));
    const int N_CONV_BLOCKS = atoi(opt(argc, argv, "--blocks", "16"));
    const int BATCH_SIZE = atoi(opt(argc, argv, "--batch", "32"));          /* resnet.cu:3279 */
    int iters = atoi(opt(argc, argv, "--iters", "-1"));                      /* iterations per epoch; default: from the class counts (below), else 10 */
    const int N_EPOCHS = atoi(opt(argc, argv, "--epochs", "1"));              /* resnet.cu:3293 (40) */
    const float LEARNING_RATE = (float)atof(opt(argc, argv, "--lr", "0.0001")); /* resnet.cu:3286-3291 */
    const float WEIGHT_DECAY = (float)atof(opt(argc, argv, "--wd", "0"));
    const float EPS = (float)atof(opt(argc, argv, "--eps", "0.0000001"));
    const int SHARD_N_IMAGES = atoi(opt(argc, argv, "--shard-images", "32768"));
    const char *shards = opt(argc, argv, "--shards", NULL);
    const char *layout = opt(argc, argv, "--layout", "nchw");
    const char *shards_u8 = opt(argc, argv, "--shards-u8", NULL);
    const int DIM_IN = atoi(opt(argc, argv, "--dim-in", "256"));
    const char *augment = opt(argc, argv, "--augment", "fixed");
    const unsigned long long aug_seed = strtoull(opt(argc, argv, "--aug-seed", "0"), NULL, 10);
    double rrc_scale[2] = {0.08, 1.0}, rrc_ratio[2] = {3.0 / 4.0, 4.0 / 3.0};
    if (sscanf(opt(argc, argv, "--rrc-scale", "0.08,1"), "%lf,%lf", &rrc_scale[0], &rrc_scale[1]) != 2) { fprintf(stderr, "--rrc-scale LO,HI\n"); return 1; }
    if (opt(argc, argv, "--rrc-ratio", NULL) && sscanf(opt(argc, argv, "--rrc-ratio", ""), "%lf,%lf", &rrc_ratio[0], &rrc_ratio[1]) != 2) { fprintf(stderr, "--rrc-ratio LO,HI\n"); return 1; }
    int flip = 1;
    for (int i = 1; i < argc; i++) if (!strcmp(argv[i], "--no-flip")) flip = 0;
    const char *smoothing_arg = opt(argc, argv, "--label-smoothing", NULL), *topk_arg = opt(argc, argv, "--topk", NULL);
    int device_loss = 0;
    for (int i = 1; i < argc; i++) if (!strcmp(argv[i], "--device-loss")) device_loss = 1;
    const double MIXUP = atof(opt(argc, argv, "--mixup", "0")), CUTMIX = atof(opt(argc, argv, "--cutmix", "0")), MIX_PROB = atof(opt(argc, argv, "--mix-prob", "1"));
    const unsigned long long mix_seed = strtoull(opt(argc, argv, "--mix-seed", "0"), NULL, 10);
    const int mixing = MIXUP != 0 || CUTMIX != 0;
    const int loss_on_device = smoothing_arg || topk_arg || device_loss || mixing;
    const double ERASE_PROB = atof(opt(argc, argv, "--random-erase", "0"));
    const char *erase_mode = opt(argc, argv, "--erase-mode", "const");
    const unsigned long long erase_seed = strtoull(opt(argc, argv, "--erase-seed", "0"), NULL, 10);
    const char *auto_augment = opt(argc, argv, "--auto-augment", NULL);
    const unsigned long long ta_seed = strtoull(opt(argc, argv, "--ta-seed", "0"), NULL, 10);
    const int TOPK = atoi(topk_arg ? topk_arg : "5");
    const char *bn_momentum_arg = opt(argc, argv, "--bn-momentum", NULL), *val_u8 = opt(argc, argv, "--val-u8", NULL);
    const int VAL_DIM_IN = atoi(opt(argc, argv, "--val-dim-in", "256")), VAL_EVERY = atoi(opt(argc, argv, "--val-every", "0"));
    const int VAL_RESIZE = atoi(opt(argc, argv, "--val-resize", "0"));
    int rrc_antialias = 0;
    for (int i = 1; i < argc; i++) if (!strcmp(argv[i], "--rrc-antialias")) rrc_antialias = 1;
    const char *ema_arg = opt(argc, argv, "--ema", NULL);
    const int EMA_EVERY = atoi(opt(argc, argv, "--ema-every", "1"));
    int ema_warmup = 0;
    for (int i = 1; i < argc; i++) if (!strcmp(argv[i], "--ema-warmup")) ema_warmup = 1;
    const int ACCUM = atoi(opt(argc, argv, "--accum", "1"));
    const float ACCUM_SCALE = (float)atof(opt(argc, argv, "--accum-scale", "1"));
    const char *optimizer = opt(argc, argv, "--optimizer", "adam"), *norm_wd_arg = opt(argc, argv, "--norm-weight-decay", NULL);
    const float MOMENTUM = (float)atof(opt(argc, argv, "--momentum", "0.9"));
    const float CLIP_GRAD_NORM = (float)atof(opt(argc, argv, "--clip-grad-norm", "0"));
    const char *dump_root = opt(argc, argv, "--dump-root", NULL);
    const char *loss_log = opt(argc, argv, "--loss-log", "avg_loss_log.txt");
    const int resume_id = atoi(opt(argc, argv, "--resume", "-1"));           /* LOAD_FROM_DUMP_ID, resnet.cu:3299 */

    /* GETTING CLASS METADATA (resnet.cu:3236-3242): total_images = sum of the per-class image counts */
    char *labels_file = (char *)opt(argc, argv, "--labels-file", NULL), *synsets_file = (char *)opt(argc, argv, "--synsets-file", NULL),
         *counts_file = (char *)opt(argc, argv, "--counts-file", NULL);
    Class_Metadata *class_metadata = NULL;
    int total_images = 0;
    if (labels_file && synsets_file && counts_file) {
        class_metadata = populate_class_info(labels_file, synsets_file, counts_file, N_CLASSES);
        for (int i = 0; i < N_CLASSES; i++) total_images += class_metadata->counts[i];
        printf("class metadata: %d classes, %d images\n", N_CLASSES, total_images);
    }
    if (iters < 0) iters = class_metadata ? (int)ceil((float)total_images / BATCH_SIZE) : 10; /* resnet.cu:3309 */

    if (mi_device_count() < 1) { fprintf(stderr, "no HIP device\n"); return 1; }
    int *reductions = (int *)calloc(N_CONV_BLOCKS > 0 ? N_CONV_BLOCKS : 1, sizeof(int));
    int final_depth = 256;
    if (N_CONV_BLOCKS == 16) { reductions[3] = reductions[7] = reductions[13] = 1; final_depth = 2048; } /* :3255-3258 */
    Dims *dims = init_dimensions(INPUT_DIM, 7, 64, 2, 3, 2, N_CONV_BLOCKS, reductions, final_depth, N_CLASSES);
    MiRng *gen = mi_rng_create(1234ULL);                                      /* :3264-3267 */
    ResNet *model = init_resnet(dims, gen);
    Batch *batch = init_general_batch(BATCH_SIZE, INPUT_DIM * INPUT_DIM * 3, INPUT_DIM, SHARD_N_IMAGES);
    if (shards_u8) {
        mi_batch_source_shards_u8(batch, shards_u8, DIM_IN);
        const int mode = !strcmp(augment, "random") ? MI_AUG_RANDOM : !strcmp(augment, "center") ? MI_AUG_CENTER : MI_AUG_FIXED;
        if (!strcmp(augment, "rrc") ? mi_batch_set_augment_rrc(batch, flip, aug_seed, rrc_scale[0], rrc_scale[1], rrc_ratio[0], rrc_ratio[1])
                                    : mi_batch_set_augment(batch, mode, flip, aug_seed)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
        if (rrc_antialias && mi_batch_set_antialias(batch, 1)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    } else if (shards) mi_batch_source_shards(batch, shards, !strcmp(layout, "nhwc") ? MI_LAYOUT_NHWC : MI_LAYOUT_NCHW);
    else mi_batch_source_synthetic(batch, 1234, 1235, N_CLASSES, 4);
    if (shards || shards_u8) mi_batch_set_prefetch(batch, 1);
    Train_ResNet *trainer = init_trainer(model, batch, BATCH_SIZE, LEARNING_RATE, WEIGHT_DECAY, 0.9f, 0.999f, EPS, N_EPOCHS, "my_custom");
    if (dump_root) mi_trainer_set_dump_root(trainer, dump_root); else mi_trainer_set_dump_every(trainer, 0);
    if (strcmp(optimizer, "adam")) {
        const int kind = !strcmp(optimizer, "sgd") ? MI_OPT_SGD : !strcmp(optimizer, "lars") ? MI_OPT_LARS : -1;
        if (kind < 0) { fprintf(stderr, "--optimizer adam|sgd|lars\n"); return 1; }
        if (mi_trainer_set_optimizer(trainer, kind, MOMENTUM, 0.001f)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    }
    if (norm_wd_arg && mi_trainer_set_norm_weight_decay(trainer, (float)atof(norm_wd_arg))) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    if (CLIP_GRAD_NORM != 0 && mi_trainer_set_clip_grad_norm(trainer, CLIP_GRAD_NORM)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    if (loss_on_device && mi_trainer_set_loss(trainer, (float)atof(smoothing_arg ? smoothing_arg : "0"), TOPK,
                                              MI_LOSS_DEVICE | (device_loss ? MI_LOSS_NO_PRED_COPY : 0))) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    if (mixing && mi_trainer_set_mix(trainer, MIXUP, CUTMIX, MIX_PROB, 0.5, mix_seed)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    if (auto_augment) {
        if (strcmp(auto_augment, "ta_wide")) { fprintf(stderr, "--auto-augment ta_wide\n"); return 1; }
        if (mi_trainer_set_trivial_augment(trainer, 1, ta_seed)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    }
    if (ERASE_PROB != 0) { /* value 0 = the mean pixel (the images are mean-subtracted, not divided); std = ImageNet's in byte units */
        if (strcmp(erase_mode, "const") && strcmp(erase_mode, "noise")) { fprintf(stderr, "--erase-mode const|noise\n"); return 1; }
        const MiEraseFill fill = {!strcmp(erase_mode, "noise") ? MI_ERASE_NOISE : MI_ERASE_CONST, {0.f, 0.f, 0.f}, {58.395f, 57.12f, 57.375f}, 0};
        if (mi_trainer_set_erase(trainer, ERASE_PROB, 0.02, 0.33, 0.3, 3.3, &fill, erase_seed)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    }
    if ((bn_momentum_arg || val_u8 || ema_arg) && mi_trainer_track_running_stats(trainer, 1, (float)atof(bn_momentum_arg ? bn_momentum_arg : "0.1"))) {
        fprintf(stderr, "%s\n", mi_last_error()); return 1;
    }
    /* before a resume: overwrite_model_params then restores the averaged model and its counter from the dump, where it holds them */
    if (ema_arg && mi_trainer_set_ema(trainer, atof(ema_arg), EMA_EVERY, ema_warmup)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    /* before a resume too: a dump made inside a window holds the sum so far */
    if (ACCUM != 1 && mi_trainer_set_accumulation(trainer, ACCUM, ACCUM_SCALE)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
    if (resume_id != -1) { overwrite_trainer_hyperparams(trainer, resume_id, "my_custom"); overwrite_model_params(trainer, resume_id, "my_custom"); }

    FILE *loss_file = fopen(loss_log, "w");
    printf("iterations per epoch: %d\n", iters);
    /* the epoch loop of resnet.cu:3327-3421, including the restart position after a resume (:3324-3325) */
    const int iterations_per_epoch = iters;
    const float total_images_per_epoch = (float)BATCH_SIZE * iterations_per_epoch;
    int cur_iter_in_epoch = (trainer->cur_dump_id + 1) % iterations_per_epoch;
    int stop = 0;
    long steps_done = 0;
    MiClipRecord clip_before = {0};
    for (int epoch = trainer->cur_epoch; epoch < N_EPOCHS && !stop; epoch++) {
        float epoch_loss = 0, epoch_n_wrong = 0;
        for (int iter = cur_iter_in_epoch; iter < iterations_per_epoch; iter++) {
            load_new_batch(trainer, class_metadata, trainer->cur_batch);
            if (mi_batch_last_status(trainer->cur_batch)) { fprintf(stderr, "data source exhausted\n"); stop = 1; break; }
            forward_pass(trainer);
            const float *pred = trainer->forward_buffer->pred_cpu;
            const int *correct = trainer->cur_batch->correct_classes_cpu;
            float batch_loss = 0, batch_n_wrong = 0;
            if (loss_on_device) { /* the record the loss head left (with --device-loss pred_cpu is not even written) */
                MiLossMetrics last;
                mi_trainer_metrics(trainer, &last, NULL, 0);
                batch_loss = (float)last.loss_sum; batch_n_wrong = (float)last.wrong_top1;
            }
            for (int s = 0; s < BATCH_SIZE && !loss_on_device; s++) batch_loss += -1 * logf(pred[s * N_CLASSES + correct[s]]);
            for (int s = 0; s < BATCH_SIZE && !loss_on_device; s++) {
                const float v = pred[s * N_CLASSES + correct[s]];
                for (int c = 0; c < N_CLASSES; c++)
                    if (c != correct[s] && pred[s * N_CLASSES + c] >= v) { batch_n_wrong++; break; }
            }
            epoch_loss += batch_loss; epoch_n_wrong += batch_n_wrong;
            const float avg = batch_loss / BATCH_SIZE, acc = 100 * ((float)BATCH_SIZE - batch_n_wrong) / (float)BATCH_SIZE;
            printf("\nEpoch: %d, Batch: %d ----- Avg. Loss: %.4f, Accuracy: %.2f%%\n\n", epoch, iter, avg, acc);
            if (loss_file) { fprintf(loss_file, "%.4f\n", avg); fflush(loss_file); }
            backwards_pass(trainer);
            update_parameters(trainer);
            if (mi_last_error()[0]) { fprintf(stderr, "device error: %s\n", mi_last_error()); return 2; }
            steps_done++;
            if (val_u8 && VAL_EVERY > 0 && steps_done % VAL_EVERY == 0 && validate(trainer, val_u8, VAL_DIM_IN, VAL_RESIZE, TOPK, "step", ema_arg != NULL)) return 1;
        }
        if (stop) break;
        if (loss_on_device) {
            MiLossMetrics total;
            mi_trainer_metrics(trainer, NULL, &total, 1);
            if (total.rows > 0)
                printf("Epoch: %d ----- Images: %lld, Avg. Loss: %.4f, Top-1 error: %.2f%%, Top-%d error: %.2f%%\n", epoch, (long long)total.rows,
                       total.loss_sum / (double)total.rows, 100.0 * (double)total.wrong_top1 / (double)total.rows, TOPK,
                       100.0 * (double)total.wrong_topk / (double)total.rows);
        }
        if (CLIP_GRAD_NORM != 0) { /* the record's counters run over the whole run: this epoch's share */
            MiClipRecord clip;
            if (mi_trainer_last_clip(trainer, &clip)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
            printf("Epoch: %d ----- Avg. Loss: %.4f, Clipped updates: %lld of %lld, last gradient norm: %.4f%s\n", epoch, epoch_loss / total_images_per_epoch,
                   (long long)(clip.clipped - clip_before.clipped), (long long)(clip.updates - clip_before.updates), clip.norm,
                   clip.nonfinite ? " (not finite: left unclipped)" : "");
            clip_before = clip;
        }
        if (val_u8 && validate(trainer, val_u8, VAL_DIM_IN, VAL_RESIZE, TOPK, "epoch", ema_arg != NULL)) return 1;
        /* resnet.cu:3410-3421: per-epoch loss (a SUM over the epoch) and accuracy, rewind the data source */
        mi_trainer_end_epoch(trainer, epoch_loss, epoch_n_wrong, total_images_per_epoch);
        cur_iter_in_epoch = 0;
    }
    mi_trainer_check_errors(trainer);
    if (dump_root) dump_trainer(77777777, trainer, trainer->dump_dir);          /* :3424-3425 */
    if (loss_file) fclose(loss_file);
    destroy_trainer(trainer);
    free(reductions);
    mi_rng_destroy(gen);
    return 0;
}
