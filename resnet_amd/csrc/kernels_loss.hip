// kernels_loss.hip -- the classification head on the device: soft-max, label-smoothed cross-entropy gradient, per-row loss and rank of the
// label in one launch (loss_head_kernel), then the batch totals in a fixed order (loss_reduce_kernel).
//
// Per row r of logits x[0..L), label c, smoothing eps, u = eps / (float)L (one wave per row, as softmax_kernel):
//   mx = max x_j, s = sum expf(x_j - mx), p_j = expf(x_j - mx) / s   the operations and the reduction order of softmax_kernel
//                                                                    (kernels_misc.hip): pred has ITS bits
//   dlogits_j = p_j - t_j, t_c = (1.f - eps) + u, t_j = u            eps = 0: p - 1.f / p - 0.f, the bits of ce_deriv_kernel; batch SUM
//   row_loss  = logf(s) - (1.f - eps) z_c - u sum_j z_j, z = x - mx  shifted log-sum-exp: finite where -logf(p_c) is +inf; sum z lane-strided
//                                                                    like s (L > 1024: in double, see DESIGN.md "Loss head")
//   row_rank  = #{ j != c : p_j >= p_c } on the p values as written  ties count against the label (mi_host_loss, resnet.cu:3363-3383);
//                                                                    top-k wrong <=> rank >= k; a NaN p_c compares false: rank 0
// A label outside [0, L): no t_c term (dlogits = p - u: what ce_deriv_kernel does), row_rank = L, row_loss = NaN, nothing read outside the
// row.  Every output may be NULL: it is then neither computed nor stored.
//
// MIX (mixup / CutMix, mi_op_loss_head_mix): two labels a, b per row and one weight lam for the launch, wa = (1.f - eps) (x) lam,
// wb = (1.f - eps) (x) (1.f - lam), each product rounded on its own:
//   dlogits_j = p_j - t_j, t_j = w_j + u, w_j = (j == a ? wa : 0.f) + (j == b ? wb : 0.f)   lam = 1.f: (1.f - eps) + u on a, u elsewhere,
//                                                                    the bits above whatever b is
//   row_loss  = logf(s) - wa z_a - wb z_b - u sum_j z_j
//   row_rank  against a, the image's own label (a training-time indicator)
// a outside [0, L): as above.  b outside [0, L) with wb > 0: no t_b term, row_loss = NaN; with wb == 0 b is never looked at.
#include "mi_common.hpp"
#include "mi_device.h"

#define LOSS_REG_COLS 1024 /* a row of up to 16 elements per lane stays in registers; a longer one is read again */

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a product and a sum that stay two roundings where they meet (the pragma, not __fmul_rn / __fadd_rn: those are plain * and + to the
// compiler, which contracts them into a fused multiply-add like any other)
__device__ __forceinline__ float loss_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    const float r = a * b;
    return r;
}
__device__ __forceinline__ float loss_add_rn(float a, float b) {
#pragma clang fp contract(off)
    const float r = a + b;
    return r;
}

// REG: x_j, then expf(x_j - mx), in v[] -- one read of the row and one expf per element; the values, and the order lane `lane` adds its
// elements lane, lane + 64, ... in, are those of the re-reading form
template <bool REG, bool MIX>
__global__ void __launch_bounds__(64)
loss_head_kernel(const float *__restrict__ x, const int *__restrict__ labels, const int *__restrict__ labels_b, float lam,
                 float *__restrict__ pred, float *__restrict__ dlogits, float *__restrict__ row_loss, int *__restrict__ row_rank, int L, float eps) {
    constexpr int NV = REG ? LOSS_REG_COLS / 64 : 1;
    const int row = blockIdx.x, lane = threadIdx.x;
    const float *xr = x + (size_t)row * L;
    const int c = labels[row];
    const bool valid = c >= 0 && c < L;
    float v[NV];
    float mx = -INFINITY;
    if (REG) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int j = lane + 64 * k;
            if (j < L) { v[k] = xr[j]; mx = fmaxf(mx, v[k]); }
        }
    } else {
        for (int j = lane; j < L; j += 64) mx = fmaxf(mx, xr[j]);
    }
    mx = wave_max(mx);
    float s = 0.f, sz = 0.f;
    if (REG) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            if (lane + 64 * k < L) {
                const float z = v[k] - mx;
                sz += z;
                v[k] = expf(z);
                s += v[k];
            }
        }
    } else {
        double szd = 0.0; /* more than 16 terms per lane: sum z in double (s keeps softmax_kernel's fp32 order: pred has its bits) */
        for (int j = lane; j < L; j += 64) {
            const float z = xr[j] - mx;
            szd += (double)z;
            s += expf(z);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) szd += __shfl_xor(szd, o, 64);
        sz = (float)szd;
    }
    s = wave_sum(s);
    const float u = eps / (float)L, tc = (1.f - eps) + u;
    const float zc = valid ? xr[c] - mx : 0.f;
    /* MIX: the second label counts only where it carries weight; wa, wb are products rounded once (no contraction into the sums below) */
    const float wa = MIX ? loss_mul_rn(1.f - eps, lam) : 0.f, wb = MIX ? loss_mul_rn(1.f - eps, 1.f - lam) : 0.f;
    const int cb = MIX && wb > 0.f ? labels_b[row] : -1;
    const bool valid_b = cb >= 0 && cb < L, lost_b = MIX && wb > 0.f && !valid_b;
    const float pc = expf(zc) / s; /* p_c as the loop below writes it */
    int above = 0;
#define LOSS_COLUMN(j_, e_)                                             \
    do {                                                                \
        const float p_ = (e_) / s;                                      \
        const size_t o_ = (size_t)row * L + (j_);                       \
        if (pred) pred[o_] = p_;                                        \
        if (dlogits) dlogits[o_] = p_ - (MIX ? loss_add_rn(loss_add_rn(valid && (j_) == c ? wa : 0.f, valid_b && (j_) == cb ? wb : 0.f), u) \
                                             : (valid && (j_) == c ? tc : u));                                                      \
        above += ((j_) != c && p_ >= pc) ? 1 : 0;                       \
    } while (0)
    if (REG) {
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const int j = lane + 64 * k;
            if (j < L) LOSS_COLUMN(j, v[k]);
        }
    } else {
        for (int j = lane; j < L; j += 64) LOSS_COLUMN(j, expf(xr[j] - mx));
    }
#undef LOSS_COLUMN
    if (row_rank) {
        above = wave_sum_i(above);
        if (lane == 0) row_rank[row] = valid ? above : L;
    }
    if (row_loss) {
        if (REG) sz = wave_sum(sz);
        if (MIX) {
            const float zb = valid_b ? xr[cb] - mx : 0.f;
            if (lane == 0) row_loss[row] = valid && !lost_b ? logf(s) - wa * zc - wb * zb - u * sz : __int_as_float(0x7fc00000);
        } else if (lane == 0) row_loss[row] = valid ? logf(s) - (1.f - eps) * zc - u * sz : __int_as_float(0x7fc00000);
    }
}

// The batch totals, one wave: lane l adds rows l, l + 64, ... in double, then the 6 exchange steps of wave_sum -- a fixed order, the same
// bits for the same rows.  last is overwritten, total added to (plain loads and stores of lane 0: launches on one stream are ordered)
__global__ void __launch_bounds__(64)
loss_reduce_kernel(const float *__restrict__ row_loss, const int *__restrict__ row_rank, int N, int topk, mid_loss_metrics *last,
                   mid_loss_metrics *total) {
    const int lane = threadIdx.x;
    double sum = 0.0;
    int w1 = 0, wk = 0;
    for (int r = lane; r < N; r += 64) {
        sum += (double)row_loss[r];
        w1 += row_rank[r] >= 1 ? 1 : 0;
        wk += row_rank[r] >= topk ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    w1 = wave_sum_i(w1);
    wk = wave_sum_i(wk);
    if (lane != 0) return;
    if (last) { last->loss_sum = sum; last->rows = N; last->wrong_top1 = w1; last->wrong_topk = wk; last->batches = 1; }
    if (total) { total->loss_sum += sum; total->rows += N; total->wrong_top1 += w1; total->wrong_topk += wk; total->batches += 1; }
}

// labels_b == NULL: the one-label head; else the two-label head with the launch's weight lam
static int loss_head_launch(const char *who, mid_stream s, const float *logits, const int *labels, const int *labels_b, float lam, float *pred,
                            float *dlogits, float *row_loss, int *row_rank, int N, int L, float smoothing, int topk, mid_loss_metrics *last_dev,
                            mid_loss_metrics *total_dev) {
    const bool reg = L <= LOSS_REG_COLS;
    if ((last_dev || total_dev) && !(row_loss && row_rank)) {
        mi_record_error(who, "the batch totals are taken from row_loss and row_rank: neither may be NULL with them");
        return -1;
    }
#define LOSS_LAUNCH(REG_, MIX_) \
    hipLaunchKernelGGL((loss_head_kernel<REG_, MIX_>), dim3(N), dim3(64), 0, (hipStream_t)s, logits, labels, labels_b, lam, pred, dlogits, row_loss, row_rank, L, smoothing)
    if (labels_b) {
        if (reg) LOSS_LAUNCH(true, true); else LOSS_LAUNCH(false, true);
        MI_LAUNCH_CHECK(reg ? "loss_head_mix_kernel<reg>" : "loss_head_mix_kernel<mem>");
    } else {
        if (reg) LOSS_LAUNCH(true, false); else LOSS_LAUNCH(false, false);
        MI_LAUNCH_CHECK(reg ? "loss_head_kernel<reg>" : "loss_head_kernel<mem>");
    }
#undef LOSS_LAUNCH
    if (last_dev || total_dev) {
        hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, row_loss, row_rank, N, topk, last_dev, total_dev);
        MI_LAUNCH_CHECK("loss_reduce_kernel");
    }
    return 0;
}
extern "C" int mid_loss_head(mid_stream s, const float *logits, const int *labels, float *pred, float *dlogits, float *row_loss, int *row_rank,
                             int N, int L, float smoothing, int topk, mid_loss_metrics *last_dev, mid_loss_metrics *total_dev) {
    return loss_head_launch("mid_loss_head", s, logits, labels, NULL, 1.f, pred, dlogits, row_loss, row_rank, N, L, smoothing, topk, last_dev, total_dev);
}
extern "C" int mid_loss_head_mix(mid_stream s, const float *logits, const int *labels_a, const int *labels_b, float lam, float *pred, float *dlogits,
                                 float *row_loss, int *row_rank, int N, int L, float smoothing, int topk, mid_loss_metrics *last_dev,
                                 mid_loss_metrics *total_dev) {
    if (!labels_b) { mi_record_error("mid_loss_head_mix", "labels_b is NULL"); return -1; }
    return loss_head_launch("mid_loss_head_mix", s, logits, labels_a, labels_b, lam, pred, dlogits, row_loss, row_rank, N, L, smoothing, topk, last_dev,
                            total_dev);
}
