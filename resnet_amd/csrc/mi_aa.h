/* mi_aa.h -- the tap table of the antialiased resize (include/resnet_mi.h, "antialiased resize"): Pillow's Image.resize(BILINEAR) on
 * 8-bit images, one axis.  ONE definition for the host (mi_aa_coeffs, loader.c) and for the device (resample_aa_u8_kernel,
 * kernels_input.hip): both compile this text, every double operation rounded on its own -- the C files are built with contraction
 * off, the HIP compiler obeys the pragma below in the host and in the device pass alike.  tests/aaref.py restates it. */
#ifndef MI_AA_H
#define MI_AA_H
#include <math.h>

#ifdef __HIPCC__
#define MI_AA_FN __host__ __device__ static inline
#else
#define MI_AA_FN static inline
#endif

#define MI_AA_BITS 22 /* fractional bits of a coefficient: Pillow's PRECISION_BITS = 32 - 8 - 2 */

/* the taps of output index o on an axis that scales `in` source pixels to V: source pixels [*lo, *hi), 1 <= *hi - *lo <= mi_aa_ksize */
MI_AA_FN void mi_aa_bounds(int in, int V, int o, int *lo, int *hi) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double scale = (double)in / (double)V;
    const double support = scale < 1.0 ? 1.0 : scale;
    const double center = ((double)o + 0.5) * scale;
    const int a = (int)(center - support + 0.5), b = (int)(center + support + 0.5);
    *lo = a < 0 ? 0 : a;
    *hi = b > in ? in : b;
}
/* the most taps any output index of such an axis has: hi - lo < 2 support + 1 <= 2 ceil(support) + 1, Pillow's ksize.  It grows with `in` */
MI_AA_FN int mi_aa_ksize(int in, int V) {
    const int c = (in + V - 1) / V;
    return 2 * (c < 1 ? 1 : c) + 1;
}
/* K[j], j < min(hi - lo, cap): the coefficients of source pixels lo + j in 2^-22; *lo as mi_aa_bounds; returns hi - lo */
MI_AA_FN int mi_aa_taps(int in, int V, int o, int *lo, int *K, int cap) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    int hi;
    mi_aa_bounds(in, V, o, lo, &hi);
    const double scale = (double)in / (double)V;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double ss = 1.0 / fs;
    const double center = ((double)o + 0.5) * scale;
    const int xmin = *lo, count = hi - xmin;
    double ww = 0.0;
    for (int j = 0; j < count; j++) {
        const double a = fabs(((double)(j + xmin) - center + 0.5) * ss);
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int j = 0; j < count && j < cap; j++) {
        const double a = fabs(((double)(j + xmin) - center + 0.5) * ss);
        const double w = a < 1.0 ? 1.0 - a : 0.0;
        K[j] = (int)(0.5 + w / ww * 4194304.0);
    }
    return count;
}
#endif
