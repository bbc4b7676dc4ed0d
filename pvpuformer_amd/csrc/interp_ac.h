// Bilinear interpolation with align_corners=True (F.interpolate(..., mode='bilinear', align_corners=True)): the one
// per-pixel formula of vpu_upsample_ac_fwd and of the batched NoBRS kernels (evalbatch.hip), so that resizing a crop in
// either gives the same bits.  (Compiled with -ffp-contract=off: the expression order below is the rounding order.)
#pragma once

// source step between neighbouring output pixels of an in_size -> out_size resize
__device__ __forceinline__ float ac_scale(int in_size, int out_size) {
    return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
}
__device__ __forceinline__ void src_index_ac(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
    const float s = scale * (float)dst;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
}
// value at output pixel (Y, X) of plane p (row stride ld) resized from (h, w) with steps (sh, sw)
__device__ __forceinline__ float ac_sample(const float* __restrict__ p, int ld, int h, int w, float sh, float sw, int Y, int X) {
    int y0, y1, x0, x1; float ly, lx;
    src_index_ac(Y, sh, h, y0, y1, ly);
    src_index_ac(X, sw, w, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * p[y0 * ld + x0] + lx * p[y0 * ld + x1]) + ly * (hx * p[y1 * ld + x0] + lx * p[y1 * ld + x1]);
}
