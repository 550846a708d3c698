// kernels_input.hip -- the input side of the step for uint8 shards (MI_SRC_SHARDS_U8): one HBM-bound pass that turns a batch of whole
// source images (bytes, [n][dim_in][dim_in][3], pixels interleaved B,G,R as the class files hold them) into the fp32 NCHW batch the
// stems read -- crop at the per-image offsets of the augmentation plan, optional horizontal flip, B,G,R -> R,G,B planes, mean
// subtraction.  It is what mi_build_shard (shards.c:75-81, build_training_shards.c:88-144) does offline, bit for bit: the value of
// byte b at position p of a source pixel is (float)((double)(float)b - mean[p]), one rounding made from a double.  The 3 x 256
// possible values are a table the compiler evaluates in double; every workgroup keeps a copy in LDS.
#include "mi_common.hpp"
#include "mi_device.h"
#include "mi_aa.h"

#define DEC_ROWS 16     // output rows of one image per workgroup
#define DEC_THREADS 256
#define DEC_TABLE_BYTES (3 * 256 * 4)

struct DecodeTable { float v[3 * 256]; };
static constexpr DecodeTable make_decode_table() {
    DecodeTable t{};
    const double mean_of_src[3] = {123.68, 116.78, 103.94}; // subtracted from source byte 0 (B), 1 (G), 2 (R): shards.c:75
    for (int p = 0; p < 3; p++)
        for (int b = 0; b < 256; b++) t.v[p * 256 + b] = (float)((double)(float)b - mean_of_src[p]);
    return t;
}
__device__ const DecodeTable g_decode_table = make_decode_table();

// 16 aligned bytes at src + a; the last 16 bytes of the batch, cut short, are read byte-wise up to total_bytes (zeros behind them)
__device__ __forceinline__ uint4 load16_in_batch(const uint8_t *__restrict__ src, size_t a, size_t total_bytes) {
    if (a + 16 <= total_bytes) return *(const uint4 *)(src + a);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16 && a + k < total_bytes; k++) w[k >> 2] |= (uint32_t)src[a + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// grid (ceil(dim_out / DEC_ROWS), n).  A cropped source row is a span of dim_out * 3 bytes that starts at an arbitrary byte (col_off * 3
// takes every residue mod 4, an odd dim_in shifts every row): the workgroup stages each of its rows' spans in LDS with aligned 16-byte
// loads -- start rounded down (src is 16-byte aligned, so never in front of it), the one load that would cross the end of the batch
// read byte-wise up to total_bytes -- and deinterleaves from LDS: a lane takes 4 consecutive output pixels (12 bytes, 3 dwords apart
// from its neighbour's: no bank conflict) and stores 16 bytes into each of the three channel planes.  vec = 0 (dim_out % 4 != 0 or an
// unaligned out): the same quads with scalar stores; the dim_out % 4 pixels at the end of a row are scalar always.
// Offsets outside [0, dim_in - dim_out] are clamped: no plan can make the kernel read outside the batch.
__global__ void __launch_bounds__(DEC_THREADS)
decode_u8_kernel(const uint8_t *__restrict__ src, const int *__restrict__ plan, float *__restrict__ out, int dim_in, int dim_out,
                 size_t total_bytes, int CH, int vec, FastDiv fdCH, FastDiv fdQ, FastDiv fdT) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dec_smem[];
    float *tab = (float *)dec_smem;
    unsigned char *rows = dec_smem + DEC_TABLE_BYTES;
    const int tid = threadIdx.x, n = blockIdx.y, h0 = blockIdx.x * DEC_ROWS;
    const int nrows = min(DEC_ROWS, dim_out - h0);
    for (int i = tid; i < 3 * 256; i += DEC_THREADS) tab[i] = g_decode_table.v[i];
    const int R = dim_in - dim_out;
    const int ro = min(max(plan[3 * n], 0), R), co = min(max(plan[3 * n + 1], 0), R), flip = plan[3 * n + 2] != 0;
    const int span = dim_out * 3;
    const size_t row0 = (((size_t)n * dim_in + ro + h0) * dim_in + co) * 3; // first byte of the workgroup's first span
    const size_t row_pitch = (size_t)dim_in * 3;

    for (int i = tid; i < nrows * CH; i += DEC_THREADS) {
        const int r = (int)fd_div((uint32_t)i, fdCH), c = i - r * CH;
        const size_t g = row0 + (size_t)r * row_pitch;
        const size_t a = (g & ~(size_t)15) + (size_t)c * 16;
        if (a < g + span) *(uint4 *)(rows + ((size_t)r * CH + c) * 16) = load16_in_batch(src, a, total_bytes);
    }
    __syncthreads();

    const int Q = dim_out >> 2;
    const size_t plane = (size_t)dim_out * dim_out;
    float *const out_n = out + (size_t)n * 3 * plane;
    for (int i = tid; i < nrows * Q; i += DEC_THREADS) {
        const int r = (int)fd_div((uint32_t)i, fdQ), w = (i - r * Q) * 4;
        const unsigned char *L = rows + (size_t)r * CH * 16 + ((row0 + (size_t)r * row_pitch) & 15);
        float v[3][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int px = flip ? dim_out - 1 - (w + j) : w + j;
#pragma unroll
            for (int p = 0; p < 3; p++) v[p][j] = tab[p * 256 + L[px * 3 + p]];
        }
        float *o = out_n + (size_t)(h0 + r) * dim_out + w;
#pragma unroll
        for (int d = 0; d < 3; d++) { // plane d (0 = R) holds source position 2 - d
            if (vec) *(float4 *)(o + d * plane) = make_float4(v[2 - d][0], v[2 - d][1], v[2 - d][2], v[2 - d][3]);
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) o[d * plane + j] = v[2 - d][j];
            }
        }
    }
    const int T = dim_out & 3;
    for (int i = tid; i < nrows * T * 3; i += DEC_THREADS) {
        const int rd = (int)fd_div((uint32_t)i, fdT), w = 4 * Q + (i - rd * T);
        const int r = rd / 3, d = rd - 3 * r;
        const unsigned char *L = rows + (size_t)r * CH * 16 + ((row0 + (size_t)r * row_pitch) & 15);
        const int px = flip ? dim_out - 1 - w : w;
        out_n[d * plane + (size_t)(h0 + r) * dim_out + w] = tab[(2 - d) * 256 + L[px * 3 + 2 - d]];
    }
}

int mid_decode_u8(mid_stream s, const uint8_t *src, const int *plan, float *out, int n, int dim_in, int dim_out) {
    if (n < 1 || n > 65535 || dim_out < 1 || dim_in < dim_out || dim_in > 16384) { mi_record_error("mid_decode_u8", "need 1 <= n <= 65535 and 1 <= dim_out <= dim_in <= 16384"); return -1; }
    if (((uintptr_t)src & 15) != 0) { mi_record_error("mid_decode_u8", "src must be 16-byte aligned"); return -1; }
    if (((uintptr_t)out & 3) != 0 || ((uintptr_t)plan & 3) != 0) { mi_record_error("mid_decode_u8", "out / plan must be 4-byte aligned"); return -1; }
    const int CH = (dim_out * 3 + 15 + 15) / 16; // 16-byte pieces a span can touch once its start is rounded down
    const size_t lds = DEC_TABLE_BYTES + (size_t)DEC_ROWS * CH * 16;
    if (lds > 65536) { mi_record_error("mid_decode_u8", "dim_out too large for the LDS row buffers"); return -2; }
    const int vec = (dim_out & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const size_t total = (size_t)n * dim_in * dim_in * 3;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 15.0 * n * dim_out * dim_out); // algorithmic: 3 bytes in, 12 out per pixel
    hipLaunchKernelGGL(decode_u8_kernel, dim3(mi_cdiv(dim_out, DEC_ROWS), n), dim3(DEC_THREADS), lds, (hipStream_t)s, src, plan, out, dim_in,
                       dim_out, total, CH, vec, make_fastdiv((uint32_t)CH), make_fastdiv((uint32_t)(dim_out >> 2)), make_fastdiv((uint32_t)(dim_out & 3)));
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK("decode_u8_kernel");
    return 0;
}

// ---- random-resized crop: a box per image, resampled to dim_out x dim_out (bilinear, 8 fractional bits), flip, planes, mean ----
// The arithmetic is integer up to the last step and written down in include/resnet_mi.h; tests/rrcref.py restates it.
#define RS_ROWS 16      // output rows of one image per workgroup (fewer where the worst-case source rows do not fit into LDS)
#define RS_THREADS 256
#define RS_LDS_MAX 65536

// source coordinate of output index o on an axis that scales `len` source pixels to D output pixels, in 1/256 pixels:
// floor(clamp((2 o + 1) len - D, 0, (len - 1) 2 D) * 256 / (2 D)).  32-bit throughout: o < D <= 16384 and len <= 16384 keep
// (2 o + 1) len below 2^29; with num = q D + r the quotient is q * 128 + (r * 128) / D, r * 128 < 2^21, the result <= (len - 1) * 256 < 2^22.
__device__ __forceinline__ int rs_coord(int o, int len, int D) {
    const int num = min(max((2 * o + 1) * len - D, 0), (len - 1) * 2 * D);
    const int q = num / D, r = num - q * D;
    return q * 128 + (r * 128) / D;
}
// one output value from the four neighbours of byte position p in the staged rows L0 (y0) and L1 (y1); x0, x1 are byte offsets of
// the two pixels; v <= 255 * 65536 is exact, the conversion is the decode table's: one rounding made from a double
__device__ __forceinline__ float rs_value(const unsigned char *L0, const unsigned char *L1, int x0, int x1, int wx, int wy, int p) {
    const double mean_of_src[3] = {123.68, 116.78, 103.94}; // as g_decode_table
    const int top = L0[x0 + p] * (256 - wx) + L0[x1 + p] * wx;
    const int bot = L1[x0 + p] * (256 - wx) + L1[x1 + p] * wx;
    return (float)((double)(top * (256 - wy) + bot * wy) * 0x1p-16 - mean_of_src[p]);
}
// source rows a block of `rows` output rows can touch when the box is as high as the image (upscaling touches fewer): the first
// and the last output row lie (rows - 1) dim_in / D source rows apart, floor() of that spread moves by at most its ceiling, + y1
static inline int rs_src_rows(int rows, int dim_in, int D) { return mi_cdiv((long)(rows - 1) * dim_in, D) + 2; }

// grid (ceil(dim_out / R), n), R output rows per workgroup.  LDS: ctab[dim_out] (x0 | wx << 16 per output column, the flip folded in),
// rtab[R] (y0 - first staged row | wy << 16), then S row buffers of CH 16-byte pieces: source rows y0(first output row) .. y1(last) of
// the box, each the span of w * 3 bytes from its 16-byte-aligned start as in decode_u8_kernel (a wave per row, a lane per piece).  R, S
// and CH come from the launcher, sized for h = w = dim_in; the box is clamped here, so no plan reads outside its image.
__global__ void __launch_bounds__(RS_THREADS)
resample_u8_kernel(const uint8_t *__restrict__ src, const int *__restrict__ boxes, float *__restrict__ out, int dim_in, int D,
                   size_t total_bytes, int R, int S, int CH, int vec, FastDiv fdQ, FastDiv fdT) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
    uint32_t *ctab = (uint32_t *)rs_smem;
    uint32_t *rtab = ctab + ((D + 3) & ~3);
    unsigned char *rows = (unsigned char *)(rtab + ((R + 3) & ~3));
    const int tid = threadIdx.x, n = blockIdx.y, h0 = blockIdx.x * R;
    const int nrows = min(R, D - h0);
    const int *bx = boxes + 5 * (size_t)n;
    const int h = min(max(bx[2], 1), dim_in), w = min(max(bx[3], 1), dim_in);
    const int r0 = min(max(bx[0], 0), dim_in - h), c0 = min(max(bx[1], 0), dim_in - w), flip = bx[4] != 0;

    const int ya = rs_coord(h0, h, D) >> 8;
    const int yb = min((rs_coord(h0 + nrows - 1, h, D) >> 8) + 1, h - 1);
    const int nsrc = min(yb - ya + 1, S); // <= S by rs_src_rows; the min keeps LDS addressing safe whatever the arithmetic
    for (int i = tid; i < D; i += RS_THREADS) {
        const int fx = rs_coord(flip ? D - 1 - i : i, w, D);
        ctab[i] = (uint32_t)(fx >> 8) | (uint32_t)(fx & 255) << 16;
    }
    if (tid < nrows) {
        const int fy = rs_coord(h0 + tid, h, D);
        rtab[tid] = (uint32_t)min((fy >> 8) - ya, S - 1) | (uint32_t)(fy & 255) << 16;
    }
    const int span = w * 3;
    const size_t g0 = (((size_t)n * dim_in + r0 + ya) * dim_in + c0) * 3; // first byte of the first staged span
    const size_t row_pitch = (size_t)dim_in * 3;
    const int pieces = min((span + 30) >> 4, CH);
    for (int r = tid >> 6; r < nsrc; r += RS_THREADS / 64) {
        const size_t g = g0 + (size_t)r * row_pitch;
        for (int c = tid & 63; c < pieces; c += 64) {
            const size_t a = (g & ~(size_t)15) + (size_t)c * 16;
            if (a < g + span) *(uint4 *)(rows + ((size_t)r * CH + c) * 16) = load16_in_batch(src, a, total_bytes);
        }
    }
    __syncthreads();

    const int Q = D >> 2, xmax = w - 1;
    const size_t plane = (size_t)D * D;
    float *const out_n = out + (size_t)n * 3 * plane;
    for (int i = tid; i < nrows * Q; i += RS_THREADS) {
        const int r = (int)fd_div((uint32_t)i, fdQ), ox = (i - r * Q) * 4;
        const uint32_t rt = rtab[r];
        const int y0 = rt & 0xFFFF, wy = rt >> 16, y1 = min(y0 + 1, nsrc - 1);
        const unsigned char *L0 = rows + (size_t)y0 * CH * 16 + ((g0 + (size_t)y0 * row_pitch) & 15);
        const unsigned char *L1 = rows + (size_t)y1 * CH * 16 + ((g0 + (size_t)y1 * row_pitch) & 15);
        float v[3][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t ct = ctab[ox + j];
            const int x0 = (ct & 0xFFFF) * 3, wx = ct >> 16, x1 = min((int)(ct & 0xFFFF) + 1, xmax) * 3;
#pragma unroll
            for (int p = 0; p < 3; p++) v[p][j] = rs_value(L0, L1, x0, x1, wx, wy, p);
        }
        float *o = out_n + (size_t)(h0 + r) * D + ox;
#pragma unroll
        for (int d = 0; d < 3; d++) { // plane d (0 = R) holds source position 2 - d
            if (vec) *(float4 *)(o + d * plane) = make_float4(v[2 - d][0], v[2 - d][1], v[2 - d][2], v[2 - d][3]);
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) o[d * plane + j] = v[2 - d][j];
            }
        }
    }
    const int T = D & 3;
    for (int i = tid; i < nrows * T * 3; i += RS_THREADS) {
        const int rd = (int)fd_div((uint32_t)i, fdT), ox = 4 * Q + (i - rd * T);
        const int r = rd / 3, p = 2 - (rd - 3 * r);
        const uint32_t rt = rtab[r], ct = ctab[ox];
        const int y0 = rt & 0xFFFF, wy = rt >> 16, y1 = min(y0 + 1, nsrc - 1);
        const int x0 = (ct & 0xFFFF) * 3, wx = ct >> 16, x1 = min((int)(ct & 0xFFFF) + 1, xmax) * 3;
        const unsigned char *L0 = rows + (size_t)y0 * CH * 16 + ((g0 + (size_t)y0 * row_pitch) & 15);
        const unsigned char *L1 = rows + (size_t)y1 * CH * 16 + ((g0 + (size_t)y1 * row_pitch) & 15);
        out_n[(2 - p) * plane + (size_t)(h0 + r) * D + ox] = rs_value(L0, L1, x0, x1, wx, wy, p);
    }
}

int mid_resample_u8(mid_stream s, const uint8_t *src, const int *boxes, float *out, int n, int dim_in, int dim_out) {
    if (n < 1 || n > 65535 || dim_out < 1 || dim_out > 16384 || dim_in < 1 || dim_in > 16384) { mi_record_error("mid_resample_u8", "need 1 <= n <= 65535 and 1 <= dim_in, dim_out <= 16384"); return -1; }
    if (((uintptr_t)src & 15) != 0) { mi_record_error("mid_resample_u8", "src must be 16-byte aligned"); return -1; }
    if (((uintptr_t)out & 3) != 0 || ((uintptr_t)boxes & 3) != 0) { mi_record_error("mid_resample_u8", "out / boxes must be 4-byte aligned"); return -1; }
    const int CH = (dim_in * 3 + 15 + 15) / 16; // 16-byte pieces the widest span can touch once its start is rounded down
    int R = dim_out < RS_ROWS ? dim_out : RS_ROWS;
    size_t lds;
    for (;; R--) { // LDS for the worst case h = w = dim_in: the box is known on the device only
        lds = (size_t)(((dim_out + 3) & ~3) + ((R + 3) & ~3)) * 4 + (size_t)rs_src_rows(R, dim_in, dim_out) * CH * 16;
        if (lds <= RS_LDS_MAX || R == 1) break;
    }
    if (lds > RS_LDS_MAX) { mi_record_error("mid_resample_u8", "dim_in too large: the source rows of one output row do not fit into LDS"); return -2; }
    const int vec = (dim_out & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const size_t total = (size_t)n * dim_in * dim_in * 3;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 15.0 * n * dim_out * dim_out); // algorithmic, as the decode: 3 bytes in, 12 out per output pixel
    hipLaunchKernelGGL(resample_u8_kernel, dim3(mi_cdiv(dim_out, R), n), dim3(RS_THREADS), lds, (hipStream_t)s, src, boxes, out, dim_in, dim_out,
                       total, R, rs_src_rows(R, dim_in, dim_out), CH, vec, make_fastdiv((uint32_t)(dim_out >> 2)), make_fastdiv((uint32_t)(dim_out & 3)));
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK("resample_u8_kernel");
    return 0;
}

// ---- antialiased resize: the box scaled to virt x virt as Pillow's Image.resize(BILINEAR) does it on bytes, a window of it written ----
// The arithmetic is written down in include/resnet_mi.h ("antialiased resize") and restated in tests/aaref.py; the tap table is mi_aa.h's,
// the text mi_aa_coeffs compiles for the host.  Two passes, the first rounded to bytes: columns, then rows.
#define AA_ROWS 16      // output rows of one image per workgroup (fewer where the worst case does not fit into LDS)
#define AA_THREADS 256
#define AA_LDS_MAX 65536

// source rows `rows` consecutive output rows can touch on an axis in -> V: the first row's lo > c0 - s - 0.5 and the last row's
// hi <= c1 + s + 0.5 with c1 - c0 = (rows - 1) in / V and s = max(in / V, 1), so hi - lo < (rows - 1) in / V + 2 s + 1; never more than `in`.
// It grows with `in`: the launcher sizes for a box as high as the image
static inline int aa_src_rows(int rows, int in, int V) {
    const int s = in >= V ? mi_cdiv((long)(rows + 1) * in, V) + 1 : mi_cdiv((long)(rows - 1) * in, V) + 3;
    return s < in ? s : in;
}
// the decode table's conversion of a byte at source position p
__device__ __forceinline__ float aa_value(int b, int p) {
    const double mean_of_src[3] = {123.68, 116.78, 103.94}; // as g_decode_table
    return (float)((double)(float)b - mean_of_src[p]);
}

// grid (ceil(D / R), n), R rows of the window per workgroup; the window is rows [win_row, + D) x columns [win_col, + D) of the virt x virt
// image.  LDS: ctab[D] and rtab[R], entries of TS = ks + 2 ints (first tap - first staged column / row, taps, the coefficients); S raw row
// buffers of CH 16-byte pieces -- box rows lo(first output row) .. hi(last), of each the byte span of columns lo(first window column) ..
// hi(last), staged from its 16-byte-aligned start as in resample_u8_kernel; S rows of MP bytes of the horizontally filtered window
// columns (flip folded in), 3 bytes a pixel.  lo and hi never decrease with the output index, so every tap lies in what was staged.
// R, S, CH and ks come from the launcher, sized for h = w = dim_in; the box is clamped here, so no plan reads outside its image.
__global__ void __launch_bounds__(AA_THREADS)
resample_aa_u8_kernel(const uint8_t *__restrict__ src, const int *__restrict__ boxes, float *__restrict__ out, int dim_in, int D, int virt,
                      int win_row, int win_col, size_t total_bytes, int R, int S, int CH, int ks, int vec, FastDiv fdD, FastDiv fdQ, FastDiv fdT) {
    extern __shared__ __attribute__((aligned(16))) unsigned char aa_smem[];
    const int TS = ks + 2, MP = (D * 3 + 3) & ~3;
    int *ctab = (int *)aa_smem;
    int *rtab = ctab + (size_t)D * TS;
    unsigned char *raw = aa_smem + ((((size_t)D + R) * TS * 4 + 15) & ~(size_t)15);
    unsigned char *mid = raw + (size_t)S * CH * 16;
    const int tid = threadIdx.x, n = blockIdx.y, h0 = blockIdx.x * R;
    const int nrows = min(R, D - h0);
    const int *bx = boxes + 5 * (size_t)n;
    const int h = min(max(bx[2], 1), dim_in), w = min(max(bx[3], 1), dim_in);
    const int r0 = min(max(bx[0], 0), dim_in - h), c0 = min(max(bx[1], 0), dim_in - w), flip = bx[4] != 0;

    int ya, yb, xa, xb, unused;
    mi_aa_bounds(h, virt, win_row + h0, &ya, &unused);
    mi_aa_bounds(h, virt, win_row + h0 + nrows - 1, &unused, &yb);
    mi_aa_bounds(w, virt, win_col, &xa, &unused);
    mi_aa_bounds(w, virt, win_col + D - 1, &unused, &xb);
    const int nsrc = min(yb - ya, S); // <= S by aa_src_rows; the min keeps LDS addressing safe whatever the arithmetic
    for (int i = tid; i < D; i += AA_THREADS) {
        int *e = ctab + (size_t)i * TS, lo;
        const int taps = mi_aa_taps(w, virt, win_col + (flip ? D - 1 - i : i), &lo, e + 2, ks);
        e[0] = lo - xa; e[1] = min(taps, ks);
    }
    for (int i = tid; i < nrows; i += AA_THREADS) {
        int *e = rtab + (size_t)i * TS, lo;
        const int taps = mi_aa_taps(h, virt, win_row + h0 + i, &lo, e + 2, ks);
        e[0] = lo - ya; e[1] = min(taps, ks);
    }
    const int span = (xb - xa) * 3;
    const size_t g0 = (((size_t)n * dim_in + r0 + ya) * dim_in + c0 + xa) * 3; // first byte of the first staged span
    const size_t row_pitch = (size_t)dim_in * 3;
    const int pieces = min((span + 30) >> 4, CH);
    for (int r = tid >> 6; r < nsrc; r += AA_THREADS / 64) {
        const size_t g = g0 + (size_t)r * row_pitch;
        for (int c = tid & 63; c < pieces; c += 64) {
            const size_t a = (g & ~(size_t)15) + (size_t)c * 16;
            if (a < g + span) *(uint4 *)(raw + ((size_t)r * CH + c) * 16) = load16_in_batch(src, a, total_bytes);
        }
    }
    __syncthreads();

    // columns: every staged row to the D window columns, rounded to bytes
    for (int i = tid; i < nsrc * D; i += AA_THREADS) {
        const int r = (int)fd_div((uint32_t)i, fdD), ox = i - r * D;
        const int *e = ctab + (size_t)ox * TS;
        const int taps = e[1];
        const unsigned char *L = raw + (size_t)r * CH * 16 + ((g0 + (size_t)r * row_pitch) & 15) + e[0] * 3;
        int s0 = 1 << (MI_AA_BITS - 1), s1 = s0, s2 = s0;
        for (int j = 0; j < taps; j++) {
            const int k = e[2 + j];
            s0 += L[3 * j] * k; s1 += L[3 * j + 1] * k; s2 += L[3 * j + 2] * k;
        }
        unsigned char *m = mid + (size_t)r * MP + ox * 3;
        m[0] = (unsigned char)min(s0 >> MI_AA_BITS, 255); m[1] = (unsigned char)min(s1 >> MI_AA_BITS, 255); m[2] = (unsigned char)min(s2 >> MI_AA_BITS, 255);
    }
    __syncthreads();

    // rows: a lane takes 4 consecutive output pixels, 12 bytes = 3 aligned dwords of every tap's row (MP and 3 ox are multiples of 4)
    const int Q = D >> 2;
    const size_t plane = (size_t)D * D;
    float *const out_n = out + (size_t)n * 3 * plane;
    for (int i = tid; i < nrows * Q; i += AA_THREADS) {
        const int r = (int)fd_div((uint32_t)i, fdQ), ox = (i - r * Q) * 4;
        const int *e = rtab + (size_t)r * TS;
        const int taps = min(e[1], nsrc - e[0]);
        const unsigned char *M = mid + (size_t)e[0] * MP + ox * 3;
        int acc[12];
#pragma unroll
        for (int t = 0; t < 12; t++) acc[t] = 1 << (MI_AA_BITS - 1);
        for (int j = 0; j < taps; j++) {
            const int k = e[2 + j];
            const uint32_t *m4 = (const uint32_t *)(M + (size_t)j * MP);
            const uint32_t d[3] = {m4[0], m4[1], m4[2]};
#pragma unroll
            for (int t = 0; t < 12; t++) acc[t] += (int)((d[t >> 2] >> (8 * (t & 3))) & 255u) * k;
        }
        float v[3][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int p = 0; p < 3; p++) v[p][j] = aa_value(min(acc[3 * j + p] >> MI_AA_BITS, 255), p);
        }
        float *o = out_n + (size_t)(h0 + r) * D + ox;
#pragma unroll
        for (int d3 = 0; d3 < 3; d3++) { // plane d3 (0 = R) holds source position 2 - d3
            if (vec) *(float4 *)(o + d3 * plane) = make_float4(v[2 - d3][0], v[2 - d3][1], v[2 - d3][2], v[2 - d3][3]);
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) o[d3 * plane + j] = v[2 - d3][j];
            }
        }
    }
    const int T = D & 3;
    for (int i = tid; i < nrows * T * 3; i += AA_THREADS) {
        const int rd = (int)fd_div((uint32_t)i, fdT), ox = 4 * Q + (i - rd * T);
        const int r = rd / 3, p = 2 - (rd - 3 * r);
        const int *e = rtab + (size_t)r * TS;
        const int taps = min(e[1], nsrc - e[0]);
        const unsigned char *M = mid + (size_t)e[0] * MP + ox * 3 + p;
        int s = 1 << (MI_AA_BITS - 1);
        for (int j = 0; j < taps; j++) s += M[(size_t)j * MP] * e[2 + j];
        out_n[(2 - p) * plane + (size_t)(h0 + r) * D + ox] = aa_value(min(s >> MI_AA_BITS, 255), p);
    }
}

int mid_resample_aa_u8(mid_stream s, const uint8_t *src, const int *boxes, float *out, int n, int dim_in, int dim_out, int virt, int win_row,
                       int win_col) {
    const char *who = "mid_resample_aa_u8";
    if (n < 1 || n > 65535 || dim_out < 1 || dim_out > 16384 || dim_in < 1 || dim_in > 16384 || virt < 1 || virt > 16384) {
        mi_record_error(who, "need 1 <= n <= 65535 and 1 <= dim_in, dim_out, virt <= 16384"); return -1;
    }
    if (win_row < 0 || win_col < 0 || win_row > virt - dim_out || win_col > virt - dim_out) { mi_record_error(who, "the window leaves [0, virt]"); return -1; }
    if (((uintptr_t)src & 15) != 0) { mi_record_error(who, "src must be 16-byte aligned"); return -1; }
    if (((uintptr_t)out & 3) != 0 || ((uintptr_t)boxes & 3) != 0) { mi_record_error(who, "out / boxes must be 4-byte aligned"); return -1; }
    const int CH = (dim_in * 3 + 15 + 15) / 16; // 16-byte pieces the widest span can touch once its start is rounded down
    const int ks = mi_aa_ksize(dim_in, virt), MP = (dim_out * 3 + 3) & ~3;
    int R = dim_out < AA_ROWS ? dim_out : AA_ROWS;
    size_t lds;
    for (;; R--) { // LDS for the worst case h = w = dim_in: the box is known on the device only
        lds = ((((size_t)dim_out + R) * (ks + 2) * 4 + 15) & ~(size_t)15) + (size_t)aa_src_rows(R, dim_in, virt) * ((size_t)CH * 16 + MP);
        if (lds <= AA_LDS_MAX || R == 1) break;
    }
    if (lds > AA_LDS_MAX) { mi_record_error(who, "dim_in too large: tables and source rows of one output row do not fit into LDS"); return -2; }
    const int vec = (dim_out & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const size_t total = (size_t)n * dim_in * dim_in * 3;
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 15.0 * n * dim_out * dim_out); // algorithmic, as the decode: 3 bytes in, 12 out per output pixel
    hipLaunchKernelGGL(resample_aa_u8_kernel, dim3(mi_cdiv(dim_out, R), n), dim3(AA_THREADS), lds, (hipStream_t)s, src, boxes, out, dim_in, dim_out,
                       virt, win_row, win_col, total, R, aa_src_rows(R, dim_in, virt), CH, ks, vec, make_fastdiv((uint32_t)dim_out),
                       make_fastdiv((uint32_t)(dim_out >> 2)), make_fastdiv((uint32_t)(dim_out & 3)));
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK("resample_aa_u8_kernel");
    return 0;
}

// ---- mixup / CutMix: a batch mixed in place, row i with row n - 1 - i (include/resnet_mi.h, "mixing"; tests/mixref.py) ----
// A pair is closed under both operations: a thread reads the same element of both images and writes both, so there is no second
// buffer and no order between workgroups.  The middle row of an odd batch pairs with itself and is left alone (grid.y = n / 2).
#define MIX_THREADS 256
#define MIX_MAX_BLOCKS_X 128

// a' = lam (x) a (+) mu (x) b, b' = lam (x) b (+) mu (x) a: every operation rounded on its own.  The pragma, not __fmul_rn / __fadd_rn:
// those are plain * and + to the compiler, which contracts them into a fused multiply-add like any other
__device__ __forceinline__ void mix_pair(float &a, float &b, float lam, float mu) {
#pragma clang fp contract(off)
    const float la = lam * a, mb = mu * b, lb = lam * b, ma = mu * a;
    const float na = la + mb, nb = lb + ma;
    a = na; b = nb;
}
// grid (x, n / 2).  Work items of a pair: quads 16-byte groups first (0 where the images are not all 16-byte aligned), then the
// image_size - 4 quads elements behind them one by one; grid-stride over both
__global__ void __launch_bounds__(MIX_THREADS)
mixup_kernel(float *__restrict__ images, int n, size_t image_size, size_t quads, float lam, float mu) {
    float *a = images + (size_t)blockIdx.y * image_size, *b = images + (size_t)(n - 1 - (int)blockIdx.y) * image_size;
    const size_t items = quads + (image_size - 4 * quads), step = (size_t)gridDim.x * MIX_THREADS;
    for (size_t i = (size_t)blockIdx.x * MIX_THREADS + threadIdx.x; i < items; i += step) {
        if (i < quads) {
            float4 va = ((const float4 *)a)[i], vb = ((const float4 *)b)[i];
            mix_pair(va.x, vb.x, lam, mu); mix_pair(va.y, vb.y, lam, mu); mix_pair(va.z, vb.z, lam, mu); mix_pair(va.w, vb.w, lam, mu);
            ((float4 *)a)[i] = va; ((float4 *)b)[i] = vb;
        } else {
            const size_t e = 4 * quads + (i - quads);
            float va = a[e], vb = b[e];
            mix_pair(va, vb, lam, mu);
            a[e] = va; b[e] = vb;
        }
    }
}
// grid (x, n / 2), a wave per row segment: rows [y0, y1) x columns [x0, x1) of the three planes of a pair change places, as words.
// The box is clamped here (0 <= y0 <= y1 <= D, x likewise): no plan addresses outside the pair.  vec (image_size % 4 == 0: both
// images' segments start at the same offset from a 16-byte boundary): the elements up to that boundary one lane each, whole 16-byte
// groups lane-strided, the rest one lane each; else every element on its own
__global__ void __launch_bounds__(MIX_THREADS)
cutmix_kernel(float *__restrict__ images, int n, int D, int y0, int x0, int y1, int x1, int vec) {
    y0 = min(max(y0, 0), D); y1 = min(max(y1, y0), D);
    x0 = min(max(x0, 0), D); x1 = min(max(x1, x0), D);
    const int h = y1 - y0, w = x1 - x0, lane = threadIdx.x & 63;
    const size_t plane = (size_t)D * D, image_size = 3 * plane;
    uint32_t *a = (uint32_t *)images + (size_t)blockIdx.y * image_size, *b = (uint32_t *)images + (size_t)(n - 1 - (int)blockIdx.y) * image_size;
    const int waves = MIX_THREADS / 64;
    for (int sgm = blockIdx.x * waves + (threadIdx.x >> 6); sgm < 3 * h; sgm += gridDim.x * waves) {
        const int d = sgm / h, y = y0 + (sgm - d * h);
        const size_t o = (size_t)d * plane + (size_t)y * D + x0;
        uint32_t *pa = a + o, *pb = b + o;
        int head = w, nq = 0;
        if (vec) {
            head = min((int)(((16 - ((uintptr_t)pa & 15)) & 15) >> 2), w);
            nq = (w - head) >> 2;
        }
        if (lane < head) { const uint32_t t = pa[lane]; pa[lane] = pb[lane]; pb[lane] = t; }
        if (!vec) for (int e = 64 + lane; e < w; e += 64) { const uint32_t t = pa[e]; pa[e] = pb[e]; pb[e] = t; }
        else {
            uint4 *qa = (uint4 *)(pa + head), *qb = (uint4 *)(pb + head);
            for (int q = lane; q < nq; q += 64) { const uint4 t = qa[q]; qa[q] = qb[q]; qb[q] = t; }
            const int e = head + 4 * nq + lane;
            if (e < w) { const uint32_t t = pa[e]; pa[e] = pb[e]; pb[e] = t; }
        }
    }
}
// labels_b[i] = labels[n - 1 - i]: the partner's label of every row (the middle row of an odd batch: its own)
__global__ void __launch_bounds__(MIX_THREADS)
mix_labels_kernel(const int *__restrict__ labels, int *__restrict__ labels_b, int n) {
    const int i = blockIdx.x * MIX_THREADS + threadIdx.x;
    if (i < n) labels_b[i] = labels[n - 1 - i];
}

int mid_mix_batch(mid_stream s, float *images, int n, size_t image_size, int dim, int mode, float lam, int y0, int x0, int y1, int x1) {
    if (!images || n < 1 || n > 65535 || dim < 1 || dim > 16384 || image_size != (size_t)3 * dim * dim) {
        mi_record_error("mid_mix_batch", "need images, 1 <= n <= 65535, 1 <= dim <= 16384 and image_size = 3 dim^2"); return -1;
    }
    if (((uintptr_t)images & 3) != 0) { mi_record_error("mid_mix_batch", "images must be 4-byte aligned"); return -1; }
    if (mode != 0 && mode != 1 && mode != 2) { mi_record_error("mid_mix_batch", "mode is 0 (none), 1 (mixup) or 2 (CutMix)"); return -1; }
    if (mode == 1 && !(lam >= 0.f && lam <= 1.f)) { mi_record_error("mid_mix_batch", "lam lies in [0, 1]"); return -1; }
    const int pairs = n / 2;
    if (mode == 0 || pairs == 0) return 0;
    const int vec = (image_size & 3) == 0 && ((uintptr_t)images & 15) == 0;
    if (mode == 1) {
        const size_t quads = vec ? image_size / 4 : 0, items = quads + (image_size - 4 * quads);
        const size_t bx = (items + MIX_THREADS - 1) / MIX_THREADS;
        mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 6.0 * pairs * image_size, 16.0 * pairs * image_size); // both images of a pair read and written once
        hipLaunchKernelGGL(mixup_kernel, dim3((unsigned)(bx < MIX_MAX_BLOCKS_X ? bx : MIX_MAX_BLOCKS_X), pairs), dim3(MIX_THREADS), 0, (hipStream_t)s, images, n,
                           image_size, quads, lam, 1.f - lam);
        mi_prof_end((hipStream_t)s);
        MI_LAUNCH_CHECK(vec ? "mixup_kernel<vec>" : "mixup_kernel<elem>");
        return 0;
    }
    const int cy0 = min(max(y0, 0), dim), cy1 = min(max(y1, cy0), dim), cx0 = min(max(x0, 0), dim), cx1 = min(max(x1, cx0), dim); // the kernel's clamp
    const int h = cy1 - cy0, w = cx1 - cx0;
    if (h == 0 || w == 0) return 0;
    const int bx = mi_cdiv(3 * h, MIX_THREADS / 64);
    mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 16.0 * pairs * 3 * h * w); // the box of both images read and written once
    hipLaunchKernelGGL(cutmix_kernel, dim3(bx < MIX_MAX_BLOCKS_X ? bx : MIX_MAX_BLOCKS_X, pairs), dim3(MIX_THREADS), 0, (hipStream_t)s, images, n, dim, y0, x0, y1,
                       x1, vec);
    mi_prof_end((hipStream_t)s);
    MI_LAUNCH_CHECK(vec ? "cutmix_kernel<vec>" : "cutmix_kernel<elem>");
    return 0;
}
int mid_mix_labels(mid_stream s, const int *labels, int *labels_b, int n) {
    if (!labels || !labels_b || n < 1) { mi_record_error("mid_mix_labels", "need both arrays and n >= 1"); return -1; }
    hipLaunchKernelGGL(mix_labels_kernel, dim3(mi_cdiv(n, MIX_THREADS)), dim3(MIX_THREADS), 0, (hipStream_t)s, labels, labels_b, n);
    MI_LAUNCH_CHECK("mix_labels_kernel");
    return 0;
}
/* the launch geometry of mixup_kernel and cutmix_kernel, for tests and documents: [0] threads, [1] the cap on grid.x, [2] waves of a
 * workgroup.  One sweep of the capped grid: [0] [1] work items of mixup_kernel, [1] [2] row segments of cutmix_kernel */
void mid_mix_geometry(size_t out[3]) { out[0] = MIX_THREADS; out[1] = MIX_MAX_BLOCKS_X; out[2] = MIX_THREADS / 64; }

// ---- random erasing: a box per image filled in place with a constant or with noise (include/resnet_mi.h, "random erasing"; tests/eraseref.py) ----
// The boxes travel by value, as kernel arguments: four uint16 a row, ER_ROWS rows a launch (2 KB of the 4 KB a launch may carry), so there
// is no staging buffer, no copy and nothing the host has to keep alive behind the launch.
#define ER_THREADS 256
#define ER_MAX_BLOCKS_X 128
#define ER_ROWS 256
struct EraseBoxes { uint16_t v[ER_ROWS][4]; };                 // (y0, x0, h, w) of the launch's rows, clamped by the launcher
struct EraseFill { float value[3], std[3]; uint64_t seed; uint64_t first; }; // first: the noise key index of the launch's row 0

// as kernels_misc.hip, synth.c and tests/synth.py define the counter streams
__device__ __forceinline__ uint64_t er_splitmix64_at(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// Irwin-Hall: twelve 16-bit fields of three draws, their sum less its mean 12 * 65535 / 2, in units of 2^-16.  |S - 393210| < 2^20, so the
// conversion and the product with a power of two are exact: integer arithmetic up to the two roundings of er_noise
__device__ __forceinline__ float er_z(uint64_t q, uint32_t el) {
    int S = 0;
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const uint64_t g = er_splitmix64_at(q, 64 + 3 * (uint64_t)el + m);
        S += (int)(g & 0xFFFF) + (int)((g >> 16) & 0xFFFF) + (int)((g >> 32) & 0xFFFF) + (int)(g >> 48);
    }
    return (float)(S - 393210) * 0x1p-16f;
}
// value (+) std (x) z: the product and the sum rounded one by one (the pragma: see mix_pair)
__device__ __forceinline__ float er_noise(float value, float std, float z) {
#pragma clang fp contract(off)
    const float sz = std * z;
    const float r = value + sz;
    return r;
}
// grid (x, rows of the launch), a wave per row segment of the row's box; a row without a box leaves at once.  The box is clamped here
// too (y0 into [0, D], h into [0, D - y0], x likewise): no argument addresses outside the row's image.  NOISE 0: plane c's word
// everywhere; 1: a value per element from its position el = (c D + y) D + x alone.  VEC (image_size % 4 == 0, a 16-byte aligned batch):
// the elements up to the segment's first 16-byte boundary one lane each, whole 16-byte groups lane-strided, the rest one lane each;
// else every element on its own, lane-strided.  Stores only: nothing is read from the batch
template <int NOISE, int VEC>
__global__ void __launch_bounds__(ER_THREADS)
erase_kernel(float *__restrict__ images, int D, EraseBoxes boxes, EraseFill fill) {
    const uint16_t *bx = boxes.v[blockIdx.y];
    const int y0 = min((int)bx[0], D), x0 = min((int)bx[1], D);
    const int h = min((int)bx[2], D - y0), w = min((int)bx[3], D - x0);
    if (h == 0 || w == 0) return;
    const int lane = threadIdx.x & 63, waves = ER_THREADS / 64;
    const size_t plane = (size_t)D * D;
    float *const img = images + (size_t)blockIdx.y * 3 * plane;
    const uint64_t q = NOISE ? er_splitmix64_at(fill.seed, fill.first + blockIdx.y) : 0;
    for (int sgm = blockIdx.x * waves + (threadIdx.x >> 6); sgm < 3 * h; sgm += gridDim.x * waves) {
        const int c = sgm / h, y = y0 + (sgm - c * h);
        const uint32_t el0 = ((uint32_t)c * D + y) * D + x0; // < 3 * 16384^2 < 2^32
        float *const p = img + el0;
        const float val = fill.value[c], sd = fill.std[c];
        int head = 0, groups = 0;
        if (VEC) {
            head = min((int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2), w);
            groups = (w - head) >> 2;
            if (lane < head) p[lane] = NOISE ? er_noise(val, sd, er_z(q, el0 + lane)) : val;
            float4 *const p4 = (float4 *)(p + head);
            for (int k = lane; k < groups; k += 64) {
                const uint32_t el = el0 + head + 4 * k;
                p4[k] = NOISE ? make_float4(er_noise(val, sd, er_z(q, el)), er_noise(val, sd, er_z(q, el + 1)), er_noise(val, sd, er_z(q, el + 2)),
                                            er_noise(val, sd, er_z(q, el + 3)))
                              : make_float4(val, val, val, val);
            }
        }
        // VEC: the at most 3 elements behind the last group; else all w of them
        for (int i = head + 4 * groups + lane; i < w; i += 64) p[i] = NOISE ? er_noise(val, sd, er_z(q, el0 + i)) : val;
    }
}

int mid_erase_fill_ok(const char *who, int mode, const float *value, const float *std) {
    if (!value || !std) { mi_record_error(who, "value / std is NULL"); return 0; }
    if (mode != 0 && mode != 1) { mi_record_error(who, "mode is 0 (MI_ERASE_CONST) or 1 (MI_ERASE_NOISE)"); return 0; }
    for (int c = 0; c < 3; c++) {
        if (!isfinite(value[c]) || !isfinite(std[c])) { mi_record_error(who, "value and std must be finite"); return 0; }
        if (std[c] < 0.f) { mi_record_error(who, "std must not be negative"); return 0; }
    }
    return 1;
}
int mid_erase_batch(mid_stream s, float *images, int n, size_t image_size, int dim, const int *boxes_host, int mode, const float *value,
                    const float *std, uint64_t noise_seed, int64_t first_row) {
    const char *who = "mid_erase_batch";
    if (!images || !boxes_host || n < 1 || n > 65535 || dim < 1 || dim > 16384 || image_size != (size_t)3 * dim * dim) {
        mi_record_error(who, "need images, boxes, 1 <= n <= 65535, 1 <= dim <= 16384 and image_size = 3 dim^2"); return -1;
    }
    if (((uintptr_t)images & 3) != 0) { mi_record_error(who, "images must be 4-byte aligned"); return -1; }
    if (!mid_erase_fill_ok(who, mode, value, std)) return -1;
    const int vec = (image_size & 3) == 0 && ((uintptr_t)images & 15) == 0;
    EraseFill fill;
    for (int c = 0; c < 3; c++) { fill.value[c] = value[c]; fill.std[c] = std[c]; }
    fill.seed = noise_seed;
    for (int r0 = 0; r0 < n; r0 += ER_ROWS) {
        const int rows = n - r0 < ER_ROWS ? n - r0 : ER_ROWS;
        EraseBoxes bx = {};
        int hmax = 0;
        double cells = 0;
        for (int i = 0; i < rows; i++) { // the kernel's clamp, so that every field fits 16 bits
            const int *b = boxes_host + 4 * (size_t)(r0 + i);
            const int y0 = min(max(b[0], 0), dim), x0 = min(max(b[1], 0), dim);
            const int h = min(max(b[2], 0), dim - y0), w = min(max(b[3], 0), dim - x0);
            if (h == 0 || w == 0) continue;
            bx.v[i][0] = (uint16_t)y0; bx.v[i][1] = (uint16_t)x0; bx.v[i][2] = (uint16_t)h; bx.v[i][3] = (uint16_t)w;
            hmax = max(hmax, h);
            cells += (double)h * w;
        }
        if (hmax == 0) continue; // no row of this launch has a box
        fill.first = (uint64_t)first_row + (uint64_t)r0;
        const int gx = mi_cdiv(3 * hmax, ER_THREADS / 64);
        const dim3 grid(gx < ER_MAX_BLOCKS_X ? gx : ER_MAX_BLOCKS_X, rows), block(ER_THREADS);
        float *const base = images + (size_t)r0 * image_size;
        mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, 12.0 * cells); // algorithmic: three words written per cell of a box
        if (mode == 0) {
            if (vec) hipLaunchKernelGGL((erase_kernel<0, 1>), grid, block, 0, (hipStream_t)s, base, dim, bx, fill);
            else hipLaunchKernelGGL((erase_kernel<0, 0>), grid, block, 0, (hipStream_t)s, base, dim, bx, fill);
        } else {
            if (vec) hipLaunchKernelGGL((erase_kernel<1, 1>), grid, block, 0, (hipStream_t)s, base, dim, bx, fill);
            else hipLaunchKernelGGL((erase_kernel<1, 0>), grid, block, 0, (hipStream_t)s, base, dim, bx, fill);
        }
        mi_prof_end((hipStream_t)s);
        MI_LAUNCH_CHECK(mode == 0 ? (vec ? "erase_kernel<const,vec>" : "erase_kernel<const,elem>") : (vec ? "erase_kernel<noise,vec>" : "erase_kernel<noise,elem>"));
    }
    return 0;
}
/* [0] threads, [1] the cap on grid.x, [2] waves of a workgroup, [3] rows of a launch.  One sweep of the capped grid: [1] [2] row segments
 * of a row's box */
void mid_erase_geometry(size_t out[4]) { out[0] = ER_THREADS; out[1] = ER_MAX_BLOCKS_X; out[2] = ER_THREADS / 64; out[3] = ER_ROWS; }

// ---- TrivialAugmentWide: one Pillow operation per image on the fp32 batch, in place (include/resnet_mi.h, "TrivialAugmentWide"; tests/taref.py) ----
// Per pixel: decode o Pillow-op o quantise.  Two kernels over a planar uint8 staging area [n][3][D][D] and integer statistics [n][4][256]
// (histograms of R, G, B and of L) in the workspace: ta_stage_kernel quantises the rows that have an operation and counts where the
// operation needs statistics; ta_apply_kernel reads the staging area and writes the batch through the decode table.  The records travel
// by value, as kernel arguments (erase_kernel's way): six words and the op a row, TA_ROWS rows a launch.  Rows with MID_TA_IDENTITY leave
// both kernels at once: nothing of theirs is read or written.
// hipcc contracts a * b + c into an FMA by default; Pillow rounds each operation.  The blend, the smooth filter's multiply-add and the
// AutoContrast entry are small functions under `#pragma clang fp contract(off)` (not __fmul_rn / __fadd_rn: see mix_pair).
#define TA_THREADS 256
#define TA_MAX_BLOCKS_X 32
#define TA_ROWS 128
struct TaOps { uint8_t op[TA_ROWS]; };
// u: A[6] for the geometric operations; u[0] the bits of `factor` for the four blends; u[0] = arg for Posterize and Solarize
struct TaRows { int32_t u[TA_ROWS][6]; uint8_t op[TA_ROWS]; };

struct TaRecip { double v[256]; };
static constexpr TaRecip make_ta_recip() { // 255.0 / k, rounded once, by the compiler
    TaRecip t{};
    for (int k = 1; k < 256; k++) t.v[k] = 255.0 / (double)k;
    return t;
}
__device__ const TaRecip g_ta_recip = make_ta_recip();

// the fp32 of the mean g_decode_table subtracts on plane d (plane d holds source position 2 - d)
__device__ __forceinline__ float ta_mean_plane(int d) { return d == 0 ? 103.94f : d == 1 ? 116.78f : 123.68f; }
// (int)rint(clamp(v (+) mean, 0, 255)); the comparisons send a NaN to 0
__device__ __forceinline__ uint32_t ta_quantise(float v, float mean) {
    float s = v + mean;
    s = s > 0.f ? s : 0.f;
    s = s < 255.f ? s : 255.f;
    return (uint32_t)(int)rintf(s);
}
__device__ __forceinline__ uint32_t ta_luma(uint32_t r, uint32_t g, uint32_t b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }
// Pillow's ImagingBlend on bytes: t = d (+) f (x) (x (-) d); inside (0 <= f <= 1): (int)t, else clipped first
__device__ __forceinline__ uint32_t ta_blend(float d, float x, float f, bool inside) {
#pragma clang fp contract(off)
    const float diff = x - d;
    const float prod = f * diff;
    const float t = d + prod;
    if (inside) return (uint32_t)(int)t & 255u;
    return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)(int)t & 255u;
}
// acc (+) v (x) k, two roundings: one tap of the smooth filter
__device__ __forceinline__ float ta_tap(float acc, float v, float k) {
#pragma clang fp contract(off)
    const float prod = v * k;
    const float r = acc + prod;
    return r;
}
// (int)(i scale + off) in double, product and sum rounded separately, truncation toward zero: Pillow's autocontrast entry
__device__ __forceinline__ int ta_stretch(int i, double scale, double off) {
#pragma clang fp contract(off)
    const double prod = (double)i * scale;
    const double r = prod + off;
    return (int)r;
}
template <int V> __device__ __forceinline__ void ta_load_bytes(const uint8_t *p, uint32_t *b) {
    if (V == 4) {
        const uint32_t w = *(const uint32_t *)p;
#pragma unroll
        for (int j = 0; j < V; j++) b[j] = (w >> (8 * j)) & 255u;
    } else b[0] = p[0];
}

template <int V> __device__ __forceinline__ void ta_store_bytes(uint8_t *p, const uint32_t *b) {
    if (V == 4) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < V; j++) w |= b[j] << (8 * j);
        *(uint32_t *)p = w;
    } else p[0] = (uint8_t)b[0];
}

// grid (x <= TA_MAX_BLOCKS_X, rows of the launch); a thread takes V consecutive pixels of the row's image per turn, all three planes.
// V = 4 (D^2 % 4 == 0 and a 16-byte aligned batch): 16-byte loads, 4-byte stores; else V = 1.  Histograms: in LDS with integer atomics,
// the occupied bins merged into the statistics with integer atomics -- sums of integers, so the order does not matter
template <int V>
__global__ void __launch_bounds__(TA_THREADS)
ta_stage_kernel(const float *__restrict__ images, uint8_t *__restrict__ stage, uint32_t *__restrict__ stats, int D, TaOps ops) {
    __shared__ uint32_t hist[4 * 256];
    const int row = blockIdx.y, op = ops.op[row], tid = threadIdx.x;
    if (op == MID_TA_IDENTITY) return;
    const bool counted = op == MID_TA_CONTRAST || op == MID_TA_AUTOCONTRAST || op == MID_TA_EQUALIZE; // uniform in the workgroup
    if (counted) {
        for (int i = tid; i < 4 * 256; i += TA_THREADS) hist[i] = 0;
        __syncthreads();
    }
    const uint32_t plane = (uint32_t)D * D, items = plane / V; // D <= 4096: plane <= 2^24
    const float *const img = images + (size_t)row * 3 * plane;
    uint8_t *const out = stage + (size_t)row * 3 * plane;
    for (uint32_t it = blockIdx.x * TA_THREADS + tid; it < items; it += gridDim.x * TA_THREADS) {
        const uint32_t p = it * V;
        uint32_t b[3][V];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            float v[V];
            VecIO<float, V>::load(img + (size_t)d * plane + p, v);
#pragma unroll
            for (int j = 0; j < V; j++) b[d][j] = ta_quantise(v[j], ta_mean_plane(d));
            ta_store_bytes<V>(out + (size_t)d * plane + p, b[d]);
        }
        if (counted) {
#pragma unroll
            for (int j = 0; j < V; j++) {
                atomicAdd(&hist[b[0][j]], 1u);
                atomicAdd(&hist[256 + b[1][j]], 1u);
                atomicAdd(&hist[512 + b[2][j]], 1u);
                atomicAdd(&hist[768 + ta_luma(b[0][j], b[1][j], b[2][j])], 1u);
            }
        }
    }
    if (counted) {
        __syncthreads();
        for (int i = tid; i < 4 * 256; i += TA_THREADS)
            if (hist[i]) atomicAdd(&stats[(size_t)row * 1024 + i], hist[i]);
    }
}

// grid and traversal as ta_stage_kernel; the operation is uniform in the workgroup.  LDS: the decode table plane by plane, and for the
// table operations a 3 x 256 byte table built here from the record and the row's statistics (thread i builds entry i of each channel:
// TA_THREADS == 256; a scan of the channel's histogram, every lane reading the same word, gives it the lowest and highest occupied bin,
// their number and the count below i).  Three families: the table operations, the per-pixel blends (Color, Sharpness), the gather
template <int V>
__global__ void __launch_bounds__(TA_THREADS)
ta_apply_kernel(float *__restrict__ images, const uint8_t *__restrict__ stage, const uint32_t *__restrict__ stats, int D, FastDiv fdD, TaRows rows) {
    __shared__ float dec[3 * 256];
    __shared__ uint32_t h[4 * 256];
    __shared__ uint8_t lut[3 * 256];
    const int row = blockIdx.y, op = rows.op[row], tid = threadIdx.x;
    if (op == MID_TA_IDENTITY) return;
    for (int i = tid; i < 3 * 256; i += TA_THREADS) dec[i] = g_decode_table.v[(2 - (i >> 8)) * 256 + (i & 255)];
    const float f = __int_as_float(rows.u[row][0]);
    const bool inside = f >= 0.f && f <= 1.f;
    const bool table = op == MID_TA_BRIGHTNESS || op == MID_TA_CONTRAST || op == MID_TA_POSTERIZE || op == MID_TA_SOLARIZE ||
                       op == MID_TA_AUTOCONTRAST || op == MID_TA_EQUALIZE;
    const uint32_t plane = (uint32_t)D * D, items = plane / V;
    if (table) {
        const uint32_t i = (uint32_t)tid; // the entry this thread builds
        if (op == MID_TA_BRIGHTNESS) {
            const uint32_t e = ta_blend(0.f, (float)i, f, inside);
            lut[i] = lut[256 + i] = lut[512 + i] = (uint8_t)e;
        } else if (op == MID_TA_POSTERIZE) {
            lut[i] = lut[256 + i] = lut[512 + i] = (uint8_t)(i & (uint32_t)rows.u[row][0]);
        } else if (op == MID_TA_SOLARIZE) {
            lut[i] = lut[256 + i] = lut[512 + i] = (uint8_t)((int)i < rows.u[row][0] ? i : 255u - i);
        } else {
            for (int k = tid; k < 4 * 256; k += TA_THREADS) h[k] = stats[(size_t)row * 1024 + k];
            __syncthreads();
            if (op == MID_TA_CONTRAST) { // M = int(mean of L + 0.5) = (2 sum + D^2) / (2 D^2)
                uint64_t sum = 0;
                for (int j = 0; j < 256; j++) sum += (uint64_t)j * h[768 + j];
                const uint32_t M = (uint32_t)((2 * sum + plane) / (2 * (uint64_t)plane));
                const uint32_t e = ta_blend((float)M, (float)i, f, inside);
                lut[i] = lut[256 + i] = lut[512 + i] = (uint8_t)e;
            } else {
                for (int c = 0; c < 3; c++) {
                    int lo = -1, hi = -1, occupied = 0;
                    uint32_t below = 0;
                    for (int j = 0; j < 256; j++) {
                        const uint32_t hj = h[c * 256 + j];
                        if (hj) { if (lo < 0) lo = j; hi = j; occupied++; }
                        if (j < (int)i) below += hj;
                    }
                    uint32_t e = i;
                    if (op == MID_TA_AUTOCONTRAST) {
                        if (hi > lo && lo >= 0) {
                            const double scale = g_ta_recip.v[hi - lo], off = -(double)lo * scale;
                            e = (uint32_t)min(max(ta_stretch((int)i, scale, off), 0), 255);
                        }
                    } else {
                        const uint32_t step = occupied >= 2 ? (plane - h[c * 256 + hi]) / 255u : 0u;
                        if (step) e = min(255u, (step / 2 + below) / step);
                    }
                    lut[c * 256 + i] = (uint8_t)e;
                }
            }
        }
    }
    __syncthreads();
    float *const img = images + (size_t)row * 3 * plane;
    const uint8_t *const in = stage + (size_t)row * 3 * plane;
    const uint32_t A0 = (uint32_t)rows.u[row][0], A1 = (uint32_t)rows.u[row][1], A2 = (uint32_t)rows.u[row][2];
    const uint32_t A3 = (uint32_t)rows.u[row][3], A4 = (uint32_t)rows.u[row][4], A5 = (uint32_t)rows.u[row][5];
    const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0); // ImageFilter.SMOOTH: (1 1 1; 1 5 1; 1 1 1) / 13 as C floats
    for (uint32_t it = blockIdx.x * TA_THREADS + tid; it < items; it += gridDim.x * TA_THREADS) {
        const uint32_t p = it * V;
        uint32_t o[3][V];
        if (table || op == MID_TA_COLOR) {
            uint32_t b[3][V];
#pragma unroll
            for (int d = 0; d < 3; d++) ta_load_bytes<V>(in + (size_t)d * plane + p, b[d]);
#pragma unroll
            for (int j = 0; j < V; j++) {
                if (table) {
#pragma unroll
                    for (int d = 0; d < 3; d++) o[d][j] = lut[d * 256 + b[d][j]];
                } else {
                    const float L = (float)ta_luma(b[0][j], b[1][j], b[2][j]);
#pragma unroll
                    for (int d = 0; d < 3; d++) o[d][j] = ta_blend(L, (float)b[d][j], f, inside);
                }
            }
        } else {
            uint32_t y = fd_div(p, fdD), x = p - y * D;
#pragma unroll
            for (int j = 0; j < V; j++) {
                if (op == MID_TA_SHARPNESS) {
                    const bool border = y == 0 || x == 0 || y + 1 >= (uint32_t)D || x + 1 >= (uint32_t)D;
#pragma unroll
                    for (int d = 0; d < 3; d++) {
                        const uint8_t *const c = in + (size_t)d * plane + p + j;
                        float s = (float)c[0];
                        if (!border) { // 0.5f, then the nine products in row-major order, one rounding each
                            float acc = 0.5f;
#pragma unroll
                            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                                for (int dx = -1; dx <= 1; dx++)
                                    acc = ta_tap(acc, (float)c[dy * D + dx], dy == 0 && dx == 0 ? k5 : k1);
                            s = acc <= 0.f ? 0.f : acc >= 255.f ? 255.f : (float)(int)acc;
                        }
                        o[d][j] = ta_blend(s, (float)c[0], f, inside);
                    }
                } else { // Pillow's 16.16 nearest affine; sums modulo 2^32 (below 2^31 for every record of mi_ta_row), arithmetic shifts
                    const int xin = (int)(A2 + A1 * y + A0 * x) >> 16, yin = (int)(A5 + A4 * y + A3 * x) >> 16;
                    const bool ok = xin >= 0 && xin < D && yin >= 0 && yin < D;
                    const uint32_t at = ok ? (uint32_t)yin * D + xin : 0u;
#pragma unroll
                    for (int d = 0; d < 3; d++) o[d][j] = ok ? in[(size_t)d * plane + at] : 0u;
                }
                if (++x == (uint32_t)D) { x = 0; y++; }
            }
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
            float v[V];
#pragma unroll
            for (int j = 0; j < V; j++) v[j] = dec[d * 256 + o[d][j]];
            VecIO<float, V>::store(img + (size_t)d * plane + p, v);
        }
    }
}

size_t mid_ta_workspace_bytes(int n, int dim) {
    if (n < 1 || dim < 1) return 0;
    return (size_t)n * 4096 + (((size_t)n * 3 * dim * dim + 15) & ~(size_t)15);
}
int mid_trivial_augment(mid_stream s, float *images, int n, size_t image_size, int dim, const mid_ta_row *rows_host, void *workspace) {
    const char *who = "mid_trivial_augment";
    if (!images || !rows_host || !workspace || n < 1 || n > 65535 || dim < 1 || dim > 4096 || image_size != (size_t)3 * dim * dim) {
        mi_record_error(who, "need images, rows, workspace, 1 <= n <= 65535, 1 <= dim <= 4096 and image_size = 3 dim^2"); return -1;
    }
    if (((uintptr_t)images & 3) != 0) { mi_record_error(who, "images must be 4-byte aligned"); return -1; }
    if (((uintptr_t)workspace & 15) != 0) { mi_record_error(who, "workspace must be 16-byte aligned"); return -1; }
    int counted = 0;
    for (int i = 0; i < n; i++) {
        const int op = rows_host[i].op, bin = rows_host[i].bin;
        if (op < 0 || op >= MID_TA_OPS || bin < 0 || bin >= MID_TA_BINS) { mi_record_error(who, "a row's op lies in [0, 14) and its bin in [0, 31)"); return -1; }
        counted |= op == MID_TA_CONTRAST || op == MID_TA_AUTOCONTRAST || op == MID_TA_EQUALIZE;
    }
    uint32_t *const stats = (uint32_t *)workspace;
    uint8_t *const stage = (uint8_t *)workspace + (size_t)n * 4096;
    const size_t plane = (size_t)dim * dim;
    const int vec = (plane & 3) == 0 && ((uintptr_t)images & 15) == 0;
    if (counted) mid_memset(stats, 0, (size_t)n * 4096, s); // on the stream: the histograms start from zero at every call
    const long items = (long)(plane / (vec ? 4 : 1));
    const int gx = mi_cdiv(items, TA_THREADS);
    for (int r0 = 0; r0 < n; r0 += TA_ROWS) {
        const int cnt = n - r0 < TA_ROWS ? n - r0 : TA_ROWS;
        TaRows rw = {};
        TaOps ops = {};
        int active = 0;
        for (int i = 0; i < cnt; i++) {
            const mid_ta_row *r = rows_host + r0 + i;
            rw.op[i] = ops.op[i] = (uint8_t)r->op;
            active += r->op != MID_TA_IDENTITY;
            if (r->op >= MID_TA_SHEAR_X && r->op <= MID_TA_ROTATE) for (int k = 0; k < 6; k++) rw.u[i][k] = r->A[k];
            else if (r->op >= MID_TA_BRIGHTNESS && r->op <= MID_TA_SHARPNESS) { union { float f; int32_t i; } w; w.f = r->factor; rw.u[i][0] = w.i; }
            else rw.u[i][0] = r->arg;
        }
        if (!active) continue; // identity rows only: nothing to do
        const dim3 grid(gx < TA_MAX_BLOCKS_X ? gx : TA_MAX_BLOCKS_X, cnt), block(TA_THREADS);
        float *const img = images + (size_t)r0 * image_size;
        uint8_t *const stg = stage + (size_t)r0 * image_size;
        uint32_t *const st = stats + (size_t)r0 * 1024;
        const double bytes = 15.0 * (double)active * (double)plane; // algorithmic: 12 in and 3 out, then 3 in and 12 out per pixel
        mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, bytes);
        if (vec) hipLaunchKernelGGL((ta_stage_kernel<4>), grid, block, 0, (hipStream_t)s, img, stg, st, dim, ops);
        else hipLaunchKernelGGL((ta_stage_kernel<1>), grid, block, 0, (hipStream_t)s, img, stg, st, dim, ops);
        mi_prof_end((hipStream_t)s);
        MI_LAUNCH_CHECK(vec ? "ta_stage_kernel<vec>" : "ta_stage_kernel<elem>");
        mi_prof_begin((hipStream_t)s, MI_FAM_OTHER, 0, bytes);
        if (vec) hipLaunchKernelGGL((ta_apply_kernel<4>), grid, block, 0, (hipStream_t)s, img, stg, st, dim, make_fastdiv((uint32_t)dim), rw);
        else hipLaunchKernelGGL((ta_apply_kernel<1>), grid, block, 0, (hipStream_t)s, img, stg, st, dim, make_fastdiv((uint32_t)dim), rw);
        mi_prof_end((hipStream_t)s);
        MI_LAUNCH_CHECK(vec ? "ta_apply_kernel<vec>" : "ta_apply_kernel<elem>");
    }
    return 0;
}
/* [0] threads, [1] the cap on grid.x, [2] rows of a launch, [3] pixels a thread takes per turn on the 16-byte path */
void mid_ta_geometry(size_t out[4]) { out[0] = TA_THREADS; out[1] = TA_MAX_BLOCKS_X; out[2] = TA_ROWS; out[3] = 4; }
