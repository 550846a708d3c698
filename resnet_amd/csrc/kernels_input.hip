// kernels_input.hip -- the input side of the step for uint8 shards (MI_SRC_SHARDS_U8): one HBM-bound pass that turns a batch of whole
// source images (bytes, [n][dim_in][dim_in][3], pixels interleaved B,G,R as the class files hold them) into the fp32 NCHW batch the
// stems read -- crop at the per-image offsets of the augmentation plan, optional horizontal flip, B,G,R -> R,G,B planes, mean
// subtraction.  It is what mi_build_shard (shards.c:75-81, build_training_shards.c:88-144) does offline, bit for bit: the value of
// byte b at position p of a source pixel is (float)((double)(float)b - mean[p]), one rounding made from a double.  The 3 x 256
// possible values are a table the compiler evaluates in double; every workgroup keeps a copy in LDS.
#include "mi_common.hpp"
#include "mi_device.h"

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
        if (a < g + span) {
            uint4 v;
            if (a + 16 <= total_bytes) v = *(const uint4 *)(src + a);
            else { // the last 16 bytes of the batch, cut short
                uint32_t w[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16 && a + k < total_bytes; k++) w[k >> 2] |= (uint32_t)src[a + k] << (8 * (k & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4 *)(rows + ((size_t)r * CH + c) * 16) = v;
        }
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
