// kernels_optim.hip -- momentum SGD and LARS (You et al. 2017) over the parameter arena, beside the reference's Adam
// (kernels_misc.hip).  The arena is cut into chunks of at most MID_OPT_CHUNK floats that never cross a tensor boundary
// (mid_chunk table, built once per trainer on the host); every pass runs one workgroup per chunk over a chunk range, so a
// data-parallel bucket (cut at block boundaries) runs exactly its own chunks.  Tensor offsets are multiples of 4 floats:
// every chunk starts 16-B aligned and is read with float4 loads, a length that is not a multiple of 4 ends in scalar code.
//
//   norms   one workgroup per chunk: (sum w^2, sum g^2) of the chunk in double, fixed-order wave + workgroup reduction,
//           one double2 partial per chunk (no atomics: the same inputs give the same bits)
//   trust   one wave per tensor: its partials summed in a fixed order -> squared norms and the LARS trust ratio
//           (NaN: a norm is not finite, the tensor is left as it is)
//   update  one workgroup per chunk (tensor id wave-uniform): the rule, the guards, gradient clearing, the NaN flag
//
// Guards (the contract of adam_kernel): a non-finite gradient element keeps its w and b and stays in the arena, finite
// gradients are cleared; a non-finite result keeps w and b; LARS leaves a whole tensor untouched when its trust ratio is not
// finite.  *nan_flag becomes the highest offending tensor index + 1 (atomicMax on an int).
//
// In front of them, where it is on, gradient clipping by the global L2 norm ("Gradient clipping") over a chunk table of its
// own, whatever the optimizer: clip_norm_kernel, one double sum g^2 per chunk; clip_coef_kernel, one wave that sums them in a fixed order
// and writes coef = min(1, max_norm / (norm + 1e-6)) into a record in device memory; clip_scale_kernel, g <- g coef where coef < 1.
//
// Behind them the two kernels of weight averaging ("Weight averaging"), which know no tensors: ema_update_kernel, e <- lerp(e,
// p, w) over a whole arena, and exchange_kernel, which swaps two arenas word for word around an eval pass on the averaged model.  In the
// same geometry grad_accum_kernel ("Gradient accumulation"): the gradient arenas of k micro-batches summed in a second arena
// and folded back, scaled, into the gradient arena in front of one optimizer update.
#include "mi_common.hpp"
#include "mi_device.h"

#define OPT_THREADS 256

__device__ __forceinline__ bool fin(float x) { return !(isnan(x) || isinf(x)); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(OPT_THREADS)
optim_norm_kernel(const float *__restrict__ p, const float *__restrict__ g, const mid_chunk *__restrict__ chunks, int c0,
                  double2 *__restrict__ part) {
    const mid_chunk ch = chunks[c0 + blockIdx.x];
    const float *pw = p + ch.start, *pg = g + ch.start;
    const int n4 = ch.len >> 2;
    double sw = 0.0, sg = 0.0;
    if (n4 == MID_OPT_CHUNK / 4) { // a whole chunk: every load in flight before the first product
        float4 w[MID_OPT_CHUNK / 4 / OPT_THREADS], q[MID_OPT_CHUNK / 4 / OPT_THREADS];
#pragma unroll
        for (int k = 0; k < MID_OPT_CHUNK / 4 / OPT_THREADS; k++) {
            w[k] = ((const float4 *)pw)[threadIdx.x + k * OPT_THREADS];
            q[k] = ((const float4 *)pg)[threadIdx.x + k * OPT_THREADS];
        }
#pragma unroll
        for (int k = 0; k < MID_OPT_CHUNK / 4 / OPT_THREADS; k++) {
            sw = fma((double)w[k].x, (double)w[k].x, sw); sw = fma((double)w[k].y, (double)w[k].y, sw);
            sw = fma((double)w[k].z, (double)w[k].z, sw); sw = fma((double)w[k].w, (double)w[k].w, sw);
            sg = fma((double)q[k].x, (double)q[k].x, sg); sg = fma((double)q[k].y, (double)q[k].y, sg);
            sg = fma((double)q[k].z, (double)q[k].z, sg); sg = fma((double)q[k].w, (double)q[k].w, sg);
        }
    } else {
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
            const float4 w = ((const float4 *)pw)[i], q = ((const float4 *)pg)[i];
            sw = fma((double)w.x, (double)w.x, sw); sw = fma((double)w.y, (double)w.y, sw);
            sw = fma((double)w.z, (double)w.z, sw); sw = fma((double)w.w, (double)w.w, sw);
            sg = fma((double)q.x, (double)q.x, sg); sg = fma((double)q.y, (double)q.y, sg);
            sg = fma((double)q.z, (double)q.z, sg); sg = fma((double)q.w, (double)q.w, sg);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < ch.len; i += OPT_THREADS) {
            sw = fma((double)pw[i], (double)pw[i], sw);
            sg = fma((double)pg[i], (double)pg[i], sg);
        }
    }
    // float squares are exact in double; the sums of a chunk are exact to ~1e-16 relative
    sw = wave_sum_d(sw);
    sg = wave_sum_d(sg);
    __shared__ double red[2][OPT_THREADS / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = sw; red[1][wave] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < OPT_THREADS / 64; k++) { a += red[0][k]; b += red[1][k]; }
        part[c0 + blockIdx.x] = make_double2(a, b);
    }
}

// one wave per tensor: lane l sums partials l, l + 64, ... in order, then a butterfly (every lane ends with the same bits).  A
// tensor has up to ~300 chunks; one thread walking them would wait on each load in turn
__global__ void __launch_bounds__(64)
optim_trust_kernel(const double2 *__restrict__ part, const int *__restrict__ first_chunk, const int *__restrict__ is_weight, int t0,
                   float trust_coef, float wd, double2 *__restrict__ sq, float *__restrict__ trust) {
    const int t = t0 + blockIdx.x;
    double sw = 0.0, sg = 0.0;
    for (int c = first_chunk[t] + threadIdx.x; c < first_chunk[t + 1]; c += 64) { sw += part[c].x; sg += part[c].y; }
    sw = wave_sum_d(sw);
    sg = wave_sum_d(sg);
    if (threadIdx.x) return;
    sq[t] = make_double2(sw, sg);
    float tr = 1.f;
    if (isnan(sw) || isinf(sw) || isnan(sg) || isinf(sg)) tr = NAN;
    else if (is_weight[t]) {
        const float wn = (float)sqrt(sw), gn = (float)sqrt(sg);
        if (wn > 0.f && gn > 0.f) tr = trust_coef * wn / (gn + wd * wn);
    }
    trust[t] = tr;
}

// KIND MID_OPT_SGD:  d = g + wd w;  b = mu b + d;  w = w - lr b                (torch.optim.SGD, dampening 0, no Nesterov; BN gamma /
//                    beta: wd_norm in place of wd, a second parameter group)
// KIND MID_OPT_LARS: b = mu b + (lr trust) (g + wd w);  w = w - b             (BN gamma / beta: trust 1, no weight decay)
template <int KIND>
__device__ __forceinline__ void opt_elem(float &w, float &gr, float &b, float s, float wdt, float lr, float mu, bool skip, bool &bad) {
    if (!fin(gr)) { bad = true; return; } // w, b kept; the gradient stays for the diagnostic dump
    if (!skip) {
        const float d = gr + wdt * w;
        float nb, nw;
        if (KIND == MID_OPT_SGD) { nb = mu * b + d; nw = w - lr * nb; }
        else { nb = mu * b + s * d; nw = w - nb; }
        if (fin(nb) && fin(nw)) { b = nb; w = nw; }
        else bad = true;
    }
    gr = 0.f;
}

template <int KIND>
__global__ void __launch_bounds__(OPT_THREADS)
optim_update_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ bm, const mid_chunk *__restrict__ chunks,
                    int c0, const int *__restrict__ is_weight, const float *__restrict__ trust, float lr, float wd, float wd_norm, float mu,
                    int *__restrict__ nan_flag) {
    const mid_chunk ch = chunks[c0 + blockIdx.x];
    const int t = ch.tensor;
    float s = lr, wdt = wd;
    bool skip = false;
    if (KIND == MID_OPT_LARS) {
        const float tr = trust[t];
        skip = !fin(tr);
        if (is_weight[t]) s = lr * tr;
        else wdt = 0.f;
    } else if (!is_weight[t]) wdt = wd_norm;
    bool bad = skip;
    float *pw = p + ch.start, *pg = g + ch.start, *pb = bm + ch.start;
    const int n4 = ch.len >> 2;
    if (n4 == MID_OPT_CHUNK / 4) { // a whole chunk: every load in flight before the first update
        constexpr int K = MID_OPT_CHUNK / 4 / OPT_THREADS;
        float4 w[K], q[K], b[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int i = threadIdx.x + k * OPT_THREADS;
            w[k] = ((float4 *)pw)[i]; q[k] = ((float4 *)pg)[i]; b[k] = ((float4 *)pb)[i];
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            opt_elem<KIND>(w[k].x, q[k].x, b[k].x, s, wdt, lr, mu, skip, bad);
            opt_elem<KIND>(w[k].y, q[k].y, b[k].y, s, wdt, lr, mu, skip, bad);
            opt_elem<KIND>(w[k].z, q[k].z, b[k].z, s, wdt, lr, mu, skip, bad);
            opt_elem<KIND>(w[k].w, q[k].w, b[k].w, s, wdt, lr, mu, skip, bad);
            const int i = threadIdx.x + k * OPT_THREADS;
            ((float4 *)pw)[i] = w[k]; ((float4 *)pg)[i] = q[k]; ((float4 *)pb)[i] = b[k];
        }
    } else {
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
            float4 w = ((float4 *)pw)[i], q = ((float4 *)pg)[i], b = ((float4 *)pb)[i];
            opt_elem<KIND>(w.x, q.x, b.x, s, wdt, lr, mu, skip, bad);
            opt_elem<KIND>(w.y, q.y, b.y, s, wdt, lr, mu, skip, bad);
            opt_elem<KIND>(w.z, q.z, b.z, s, wdt, lr, mu, skip, bad);
            opt_elem<KIND>(w.w, q.w, b.w, s, wdt, lr, mu, skip, bad);
            ((float4 *)pw)[i] = w; ((float4 *)pg)[i] = q; ((float4 *)pb)[i] = b;
        }
    }
    for (int i = (n4 << 2) + threadIdx.x; i < ch.len; i += OPT_THREADS) {
        float w = pw[i], q = pg[i], b = pb[i];
        opt_elem<KIND>(w, q, b, s, wdt, lr, mu, skip, bad);
        pw[i] = w; pg[i] = q; pb[i] = b;
    }
    if (bad && nan_flag) atomicMax(nan_flag, t + 1);
}

// ---- gradient clipping by the global L2 norm ("Gradient clipping"): three launches over a chunk table that covers every tensor
// of the gradient arena and none of its padding.  No atomics: the same gradient gives the same record and the same scaled bits ----
// sum g^2 of one chunk in double (a float's square is exact there); reads g only
__global__ void __launch_bounds__(OPT_THREADS)
clip_norm_kernel(const float *__restrict__ g, const mid_chunk *__restrict__ chunks, double *__restrict__ part) {
    const mid_chunk ch = chunks[blockIdx.x];
    const float *src = g + ch.start;
    const int n4 = ch.len >> 2;
    double acc = 0.0;
    if (n4 == MID_OPT_CHUNK / 4) { // a whole chunk: every load in flight before the first product
        constexpr int K = MID_OPT_CHUNK / 4 / OPT_THREADS;
        float4 v[K];
#pragma unroll
        for (int k = 0; k < K; k++) v[k] = ((const float4 *)src)[threadIdx.x + k * OPT_THREADS];
#pragma unroll
        for (int k = 0; k < K; k++) {
            acc = fma((double)v[k].x, (double)v[k].x, acc); acc = fma((double)v[k].y, (double)v[k].y, acc);
            acc = fma((double)v[k].z, (double)v[k].z, acc); acc = fma((double)v[k].w, (double)v[k].w, acc);
        }
    } else {
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
            const float4 v = ((const float4 *)src)[i];
            acc = fma((double)v.x, (double)v.x, acc); acc = fma((double)v.y, (double)v.y, acc);
            acc = fma((double)v.z, (double)v.z, acc); acc = fma((double)v.w, (double)v.w, acc);
        }
        for (int i = (n4 << 2) + threadIdx.x; i < ch.len; i += OPT_THREADS) acc = fma((double)src[i], (double)src[i], acc);
    }
    acc = wave_sum_d(acc);
    __shared__ double wave_acc[OPT_THREADS / 64];
    if ((threadIdx.x & 63) == 0) wave_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < OPT_THREADS / 64; k++) total += wave_acc[k];
        part[blockIdx.x] = total;
    }
}

// one wave: lane l sums partials l, l + 64, ... in order (ResNet-50: 5910 partials, 93 turns), then the butterfly; lane 0 writes the
// record.  A sum that is not finite leaves the gradient to the optimizers' own guards: coef 1, nonfinite 1 (torch.nn.utils.clip_grad_norm_
// would multiply every gradient by NaN)
__global__ void __launch_bounds__(64)
clip_coef_kernel(const double *__restrict__ part, int n_chunks, float max_norm, mid_clip_record *__restrict__ rec) {
    double sq = 0.0;
    for (int c = threadIdx.x; c < n_chunks; c += 64) sq += part[c];
    sq = wave_sum_d(sq);
    if (threadIdx.x) return;
    const bool bad = isnan(sq) || isinf(sq);
    const double norm = sqrt(sq);
    float coef = 1.f;
    if (!bad) {
        const double r = (double)max_norm / (norm + 1e-6);
        if (r < 1.0) coef = (float)r; // rounded once; a ratio within half an ulp of 1 rounds to 1.f: not clipped
    }
    rec->sq_norm = sq; rec->norm = norm; rec->coef = coef; rec->nonfinite = bad;
    rec->updates += 1;
    if (coef < 1.f) rec->clipped += 1;
}

// g <- g coef, one fp32 product per element; coef == 1: no gradient word is read or written
__global__ void __launch_bounds__(OPT_THREADS)
clip_scale_kernel(float *__restrict__ g, const mid_chunk *__restrict__ chunks, const mid_clip_record *__restrict__ rec) {
    const float coef = rec->coef;
    if (coef == 1.0f) return;
    const mid_chunk ch = chunks[blockIdx.x];
    float *dst = g + ch.start;
    const int n4 = ch.len >> 2;
    if (n4 == MID_OPT_CHUNK / 4) { // a whole chunk: every load in flight before the first store
        constexpr int K = MID_OPT_CHUNK / 4 / OPT_THREADS;
        float4 v[K];
#pragma unroll
        for (int k = 0; k < K; k++) v[k] = ((const float4 *)dst)[threadIdx.x + k * OPT_THREADS];
#pragma unroll
        for (int k = 0; k < K; k++) {
            v[k].x *= coef; v[k].y *= coef; v[k].z *= coef; v[k].w *= coef;
            ((float4 *)dst)[threadIdx.x + k * OPT_THREADS] = v[k];
        }
    } else {
        for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
            float4 v = ((const float4 *)dst)[i];
            v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
            ((float4 *)dst)[i] = v;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < ch.len; i += OPT_THREADS) dst[i] *= coef;
    }
}

// ---- weight averaging: the EMA of an arena and the exchange of two arenas.  Pure streaming, no tensor table: a workgroup's turn is
// EMA_TURN items of V floats (V = 4: 16-byte accesses, both pointers 16-byte aligned; V = 1: any 4-byte aligned pair), every load of a
// whole turn in flight before the first use, a grid of at most EMA_MAX_GRID workgroups striding over 64-bit item indices.  The n % 4
// floats behind the last float4 are the first workgroup's, element-wise ----
#define EMA_PER_THREAD 4
#define EMA_TURN (OPT_THREADS * EMA_PER_THREAD)
#define EMA_MAX_GRID 2048
#define EMA_MAX_N ((size_t)1 << 40)

// torch.lerp(e, p, w) with its products contracted: the difference rounded once, then one fma on either side of w = 0.5 (omw = 1.f - w,
// rounded once).  A result that is not finite (p or e is not, or the difference overflows) leaves the element as it is
__device__ __forceinline__ float ema_elem(float e, float pv, float w, float omw) {
    const float d = pv - e;
    const float r = w < 0.5f ? fmaf(w, d, e) : fmaf(-omw, d, pv);
    return fin(r) ? r : e;
}

template <int V>
__global__ void __launch_bounds__(OPT_THREADS)
ema_update_kernel(float *__restrict__ ema, const float *__restrict__ p, size_t n, float w) {
    const float omw = 1.f - w;
    const size_t items = n / V, stride = (size_t)gridDim.x * EMA_TURN;
    for (size_t base = (size_t)blockIdx.x * EMA_TURN; base < items; base += stride) {
        float e[EMA_PER_THREAD][V], q[EMA_PER_THREAD][V];
        if (base + EMA_TURN <= items) { // a whole turn: every load in flight before the first update
#pragma unroll
            for (int k = 0; k < EMA_PER_THREAD; k++) {
                const size_t i = (base + threadIdx.x + k * OPT_THREADS) * V;
                VecIO<float, V>::load(ema + i, e[k]); VecIO<float, V>::load(p + i, q[k]);
            }
#pragma unroll
            for (int k = 0; k < EMA_PER_THREAD; k++) {
#pragma unroll
                for (int j = 0; j < V; j++) e[k][j] = ema_elem(e[k][j], q[k][j], w, omw);
                VecIO<float, V>::store(ema + (base + threadIdx.x + k * OPT_THREADS) * V, e[k]);
            }
        } else {
            for (size_t it = base + threadIdx.x; it < items; it += OPT_THREADS) {
                VecIO<float, V>::load(ema + it * V, e[0]); VecIO<float, V>::load(p + it * V, q[0]);
#pragma unroll
                for (int j = 0; j < V; j++) e[0][j] = ema_elem(e[0][j], q[0][j], w, omw);
                VecIO<float, V>::store(ema + it * V, e[0]);
            }
        }
    }
    if (V > 1 && blockIdx.x == 0) {
        const size_t i = items * V + threadIdx.x;
        if (i < n) ema[i] = ema_elem(ema[i], p[i], w, omw);
    }
}

// a <-> b as 32-bit words: no arithmetic touches a value, NaN payloads and -0 change places as they are
template <int V> struct ExWord;
template <> struct ExWord<1> { typedef uint32_t T; };
template <> struct ExWord<4> { typedef uint4 T; };
template <int V>
__global__ void __launch_bounds__(OPT_THREADS)
exchange_kernel(uint32_t *__restrict__ a, uint32_t *__restrict__ b, size_t n) {
    typedef typename ExWord<V>::T T;
    T *av = (T *)a, *bv = (T *)b;
    const size_t items = n / V, stride = (size_t)gridDim.x * EMA_TURN;
    for (size_t base = (size_t)blockIdx.x * EMA_TURN; base < items; base += stride) {
        if (base + EMA_TURN <= items) {
            T x[EMA_PER_THREAD], y[EMA_PER_THREAD];
#pragma unroll
            for (int k = 0; k < EMA_PER_THREAD; k++) {
                const size_t i = base + threadIdx.x + k * OPT_THREADS;
                x[k] = av[i]; y[k] = bv[i];
            }
#pragma unroll
            for (int k = 0; k < EMA_PER_THREAD; k++) {
                const size_t i = base + threadIdx.x + k * OPT_THREADS;
                av[i] = y[k]; bv[i] = x[k];
            }
        } else {
            for (size_t it = base + threadIdx.x; it < items; it += OPT_THREADS) {
                const T x = av[it], y = bv[it];
                av[it] = y; bv[it] = x;
            }
        }
    }
    if (V > 1 && blockIdx.x == 0) {
        const size_t i = items * V + threadIdx.x;
        if (i < n) { const uint32_t x = a[i], y = b[i]; a[i] = y; b[i] = x; }
    }
}

// ---- gradient accumulation ("Gradient accumulation"): the sum of k micro-batch gradient arenas, in the geometry above.  acc and
// g are arenas of n words; MODE first: acc <- g as words (no arithmetic touches a value), add: acc <- acc (+) g, fold: g <- (acc (+) g) (x)
// scale with acc only read.  Every operation is rounded on its own and nothing is guarded: what IEEE gives for a value that is not finite
// is what the optimizer behind the fold sees ----
// the pragma, not __fadd_rn / __fmul_rn (mix_pair, kernels_input.hip): the fold's sum and product must stay two roundings
template <int MODE>
__device__ __forceinline__ uint32_t acc_word(uint32_t a, uint32_t q, float scale) {
#pragma clang fp contract(off)
    if (MODE == MID_ACC_FIRST) return q;
    const float sum = __uint_as_float(a) + __uint_as_float(q);
    if (MODE == MID_ACC_ADD) return __float_as_uint(sum);
    const float scaled = sum * scale;
    return __float_as_uint(scaled);
}
template <int MODE> __device__ __forceinline__ uint32_t acc_item(uint32_t a, uint32_t q, float scale) { return acc_word<MODE>(a, q, scale); }
template <int MODE> __device__ __forceinline__ uint4 acc_item(uint4 a, uint4 q, float scale) {
    return make_uint4(acc_word<MODE>(a.x, q.x, scale), acc_word<MODE>(a.y, q.y, scale), acc_word<MODE>(a.z, q.z, scale), acc_word<MODE>(a.w, q.w, scale));
}

template <int V, int MODE>
__global__ void __launch_bounds__(OPT_THREADS)
grad_accum_kernel(uint32_t *__restrict__ acc, uint32_t *__restrict__ g, size_t n, float scale) {
    typedef typename ExWord<V>::T T;
    constexpr bool READS_ACC = MODE != MID_ACC_FIRST;
    const T *av = (const T *)acc, *gv = (const T *)g;
    T *out = (T *)(MODE == MID_ACC_FOLD ? g : acc);
    const size_t items = n / V, stride = (size_t)gridDim.x * EMA_TURN;
    for (size_t base = (size_t)blockIdx.x * EMA_TURN; base < items; base += stride) {
        if (base + EMA_TURN <= items) { // a whole turn: every load in flight before the first store
            T x[EMA_PER_THREAD], y[EMA_PER_THREAD];
#pragma unroll
            for (int k = 0; k < EMA_PER_THREAD; k++) {
                const size_t i = base + threadIdx.x + k * OPT_THREADS;
                y[k] = gv[i];
                x[k] = READS_ACC ? av[i] : y[k];
            }
#pragma unroll
            for (int k = 0; k < EMA_PER_THREAD; k++) out[base + threadIdx.x + k * OPT_THREADS] = acc_item<MODE>(x[k], y[k], scale);
        } else {
            for (size_t it = base + threadIdx.x; it < items; it += OPT_THREADS) {
                const T y = gv[it], x = READS_ACC ? av[it] : y;
                out[it] = acc_item<MODE>(x, y, scale);
            }
        }
    }
    if (V > 1 && blockIdx.x == 0) {
        const size_t i = items * V + threadIdx.x;
        if (i < n) {
            const uint32_t y = g[i], x = READS_ACC ? acc[i] : y;
            (MODE == MID_ACC_FOLD ? g : acc)[i] = acc_word<MODE>(x, y, scale);
        }
    }
}

// the grid of all three: one workgroup per turn of V-float items, capped (n >= 1)
static unsigned ema_grid(size_t n, int V) {
    const size_t turns = (n / V + EMA_TURN - 1) / EMA_TURN;
    return (unsigned)(turns < 1 ? 1 : turns > EMA_MAX_GRID ? EMA_MAX_GRID : turns);
}

template <int V>
static void accum_launch(hipStream_t st, uint32_t *acc, uint32_t *g, size_t n, int mode, float scale) {
    const dim3 grid(ema_grid(n, V)), block(OPT_THREADS);
    if (mode == MID_ACC_FIRST) hipLaunchKernelGGL((grad_accum_kernel<V, MID_ACC_FIRST>), grid, block, 0, st, acc, g, n, scale);
    else if (mode == MID_ACC_ADD) hipLaunchKernelGGL((grad_accum_kernel<V, MID_ACC_ADD>), grid, block, 0, st, acc, g, n, scale);
    else hipLaunchKernelGGL((grad_accum_kernel<V, MID_ACC_FOLD>), grid, block, 0, st, acc, g, n, scale);
}

extern "C" {
int mid_ema_update(mid_stream s, float *ema, const float *p, size_t n, float w) {
    const char *who = "mid_ema_update";
    if (!ema || !p) { mi_record_error(who, "a pointer is NULL"); return -1; }
    if ((((uintptr_t)ema | (uintptr_t)p) & 3) != 0) { mi_record_error(who, "ema / p must be 4-byte aligned"); return -1; }
    if (!(w >= 0.f && w <= 1.f)) { mi_record_error(who, "w lies in [0, 1]"); return -1; }
    if (n == 0 || n > EMA_MAX_N) { mi_record_error(who, "n lies in [1, 2^40]"); return -1; }
    const bool vec = (((uintptr_t)ema | (uintptr_t)p) & 15) == 0;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 12.0 * (double)n); // algorithmic: e and p in, e out
    if (vec) hipLaunchKernelGGL(ema_update_kernel<4>, dim3(ema_grid(n, 4)), dim3(OPT_THREADS), 0, (hipStream_t)s, ema, p, n, w);
    else hipLaunchKernelGGL(ema_update_kernel<1>, dim3(ema_grid(n, 1)), dim3(OPT_THREADS), 0, (hipStream_t)s, ema, p, n, w);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK(vec ? "ema_update_kernel<vector>" : "ema_update_kernel<element-wise>");
    return 0;
}
int mid_exchange(mid_stream s, float *a, float *b, size_t n) {
    const char *who = "mid_exchange";
    if (!a || !b) { mi_record_error(who, "a pointer is NULL"); return -1; }
    if ((((uintptr_t)a | (uintptr_t)b) & 3) != 0) { mi_record_error(who, "a / b must be 4-byte aligned"); return -1; }
    if (n == 0 || n > EMA_MAX_N) { mi_record_error(who, "n lies in [1, 2^40]"); return -1; }
    const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b, hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
    if (hi - lo < n * sizeof(float)) { mi_record_error(who, "the two ranges overlap"); return -1; }
    const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 16.0 * (double)n); // algorithmic: both in, both out
    if (vec) hipLaunchKernelGGL(exchange_kernel<4>, dim3(ema_grid(n, 4)), dim3(OPT_THREADS), 0, (hipStream_t)s, (uint32_t *)a, (uint32_t *)b, n);
    else hipLaunchKernelGGL(exchange_kernel<1>, dim3(ema_grid(n, 1)), dim3(OPT_THREADS), 0, (hipStream_t)s, (uint32_t *)a, (uint32_t *)b, n);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK(vec ? "exchange_kernel<vector>" : "exchange_kernel<element-wise>");
    return 0;
}
/* the launch geometry, for tests and documents: [0] threads, [1] floats of one workgroup's turn in the vector instantiation, [2] in the
 * element-wise one, [3] the grid's cap */
void mid_ema_geometry(size_t out[4]) { out[0] = OPT_THREADS; out[1] = (size_t)EMA_TURN * 4; out[2] = EMA_TURN; out[3] = EMA_MAX_GRID; }
int mid_grad_accumulate(mid_stream s, float *acc, float *g, size_t n, int mode, float scale) {
    static const char *const names[3][2] = {{"grad_accum_kernel<first,element-wise>", "grad_accum_kernel<first,vector>"},
                                            {"grad_accum_kernel<add,element-wise>", "grad_accum_kernel<add,vector>"},
                                            {"grad_accum_kernel<fold,element-wise>", "grad_accum_kernel<fold,vector>"}};
    const char *who = "mid_grad_accumulate";
    if (!acc || !g) { mi_record_error(who, "a pointer is NULL"); return -1; }
    if ((((uintptr_t)acc | (uintptr_t)g) & 3) != 0) { mi_record_error(who, "acc / g must be 4-byte aligned"); return -1; }
    if (n == 0 || n > EMA_MAX_N) { mi_record_error(who, "n lies in [1, 2^40]"); return -1; }
    const uintptr_t lo = (uintptr_t)acc < (uintptr_t)g ? (uintptr_t)acc : (uintptr_t)g, hi = (uintptr_t)acc < (uintptr_t)g ? (uintptr_t)g : (uintptr_t)acc;
    if (hi - lo < n * sizeof(float)) { mi_record_error(who, "the two ranges overlap"); return -1; }
    if (mode != MID_ACC_FIRST && mode != MID_ACC_ADD && mode != MID_ACC_FOLD) { mi_record_error(who, "unknown mode"); return -1; }
    if (mode == MID_ACC_FOLD && !(scale > 0.f && scale <= 3.402823466e+38f)) { mi_record_error(who, "scale is finite and > 0"); return -1; }
    const bool vec = (((uintptr_t)acc | (uintptr_t)g) & 15) == 0;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, (mode == MID_ACC_FIRST ? 8.0 : 12.0) * (double)n); // algorithmic: g (and acc) in, one out
    if (vec) accum_launch<4>((hipStream_t)s, (uint32_t *)acc, (uint32_t *)g, n, mode, scale);
    else accum_launch<1>((hipStream_t)s, (uint32_t *)acc, (uint32_t *)g, n, mode, scale);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK(names[mode][vec]);
    return 0;
}
int mid_clip_norm(mid_stream s, const float *g, const mid_chunk *chunks, int n_chunks, double *part) {
    if (n_chunks < 1) return 0;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 0); // (the bytes are the caller's to count: the launcher does not know the chunks' lengths)
    hipLaunchKernelGGL(clip_norm_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)s, g, chunks, part);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK("clip_norm_kernel");
    return 0;
}
int mid_clip_coef(mid_stream s, const double *part, int n_chunks, float max_norm, mid_clip_record *rec) {
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 8.0 * n_chunks);
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, part, n_chunks, max_norm, rec);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK("clip_coef_kernel");
    return 0;
}
int mid_clip_scale(mid_stream s, float *g, const mid_chunk *chunks, int n_chunks, const mid_clip_record *rec) {
    if (n_chunks < 1) return 0;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 0);
    hipLaunchKernelGGL(clip_scale_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)s, g, chunks, rec);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK("clip_scale_kernel");
    return 0;
}
int mid_optim_norms(mid_stream s, const float *p, const float *g, const mid_chunk *chunks, int c0, int c1, double *part) {
    if (c1 <= c0) return 0;
    hipLaunchKernelGGL(optim_norm_kernel, dim3(c1 - c0), dim3(OPT_THREADS), 0, (hipStream_t)s, p, g, chunks, c0, (double2 *)part);
    MI_LAUNCH_CHECK("optim_norm_kernel");
    return 0;
}
int mid_optim_trust(mid_stream s, const double *part, const int *first_chunk, const int *is_weight, int t0, int t1, float trust_coef,
                    float wd, double *sq, float *trust) {
    if (t1 <= t0) return 0;
    hipLaunchKernelGGL(optim_trust_kernel, dim3(t1 - t0), dim3(64), 0, (hipStream_t)s, (const double2 *)part, first_chunk, is_weight, t0,
                       trust_coef, wd, (double2 *)sq, trust);
    MI_LAUNCH_CHECK("optim_trust_kernel");
    return 0;
}
int mid_optim_update(mid_stream s, int kind, float *p, float *g, float *b, const mid_chunk *chunks, int c0, int c1, const int *is_weight,
                     const float *trust, float lr, float wd, float wd_norm, float momentum, int *nan_flag) {
    if (c1 <= c0) return 0;
    if (kind == MID_OPT_SGD)
        hipLaunchKernelGGL(optim_update_kernel<MID_OPT_SGD>, dim3(c1 - c0), dim3(OPT_THREADS), 0, (hipStream_t)s, p, g, b, chunks, c0,
                           is_weight, trust, lr, wd, wd_norm, momentum, nan_flag);
    else if (kind == MID_OPT_LARS)
        hipLaunchKernelGGL(optim_update_kernel<MID_OPT_LARS>, dim3(c1 - c0), dim3(OPT_THREADS), 0, (hipStream_t)s, p, g, b, chunks, c0,
                           is_weight, trust, lr, wd, wd_norm, momentum, nan_flag);
    else { mi_record_error("mid_optim_update", "unknown optimizer kind"); return -1; }
    MI_LAUNCH_CHECK("optim_update_kernel");
    return 0;
}
}
