// Batched NoBRS evaluation (pvpuformer_amd/isegm/inference/batched.py): K objects of different images and sizes step
// through the click loop together.  Every kernel reads a device array of per-object descriptors (vpu_eval_obj,
// include/vpu_hip.h), so that one launch covers all of them whatever their sizes.  All passes are bandwidth-bound
// streams over the objects' canvases: 4 pixels per thread (16-byte fp32 / 4-byte uint8 accesses), block-level reduction,
// one atomic per workgroup and counter.  Kernels neither allocate nor synchronise (hipGraph-capturable).
#include <cstdio>

#include "vpu_common.h"
#include "cc_union.h"
#include "interp_ac.h"
#include "../../include/vpu_hip.h"

#define ST reinterpret_cast<hipStream_t>(stream)

namespace {

// -------------------------------------------------------------------------------------------------------------------
// (0) what the paste (2), session (5) and annotation (7) passes share.
//
//     MaskRec<NSUM, GATE>: a thread's share of an int32 [8] record {NSUM pixel counts | rmin, rmax, cmin, cmax | zeros}.  The box
//     is that of the pixels sum GATE counts, and count(r, c) takes one such pixel.  The three layouts:
//       paste statistics {intersection, union, count | box}, session {area, count | box}, annotation {area, overwritten | box}.
//     rec_init writes the empty record {0.. | H, -1, W, -1 | 0..}; rec_reduce adds a block's shares to it: wave xor-shuffles, the
//     four waves' partials through LDS, then one atomic per block and counter, the box only when the block counted a pixel of it.
template <int NSUM, int GATE>
struct MaskRec {
    int sum[NSUM] = {};
    int r0 = 0x7fffffff, r1 = -1, c0 = 0x7fffffff, c1 = -1;
    __device__ __forceinline__ void count(int r, int c) {
        ++sum[GATE];
        r0 = min(r0, r); r1 = max(r1, r); c0 = min(c0, c); c1 = max(c1, c);
    }
};
using PasteRec = MaskRec<3, 2>;
using SessionRec = MaskRec<2, 1>;
using AnnotRec = MaskRec<2, 0>;
using TidyRec = MaskRec<3, 0>;

template <int NSUM>
__device__ __forceinline__ void rec_init(int* rec, int H, int W) {
#pragma unroll
    for (int k = 0; k < 8; ++k) rec[k] = 0;
    rec[NSUM] = H; rec[NSUM + 1] = -1; rec[NSUM + 2] = W; rec[NSUM + 3] = -1;
}

__device__ __forceinline__ int* rec_of(const vpu_eval_obj& d) { return reinterpret_cast<int*>(d.out + 2); }
__device__ __forceinline__ int* rec_of(const vpu_session_obj& d) { return d.rec; }
__device__ __forceinline__ int* rec_of(const vpu_annot_obj& d) { return d.rec; }
__device__ __forceinline__ int* rec_of(const vpu_tidy_obj& d) { return d.rec; }

template <int NSUM, class D>
__global__ void rec_init_kernel(const D* __restrict__ objs, int n) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < n) rec_init<NSUM>(rec_of(objs[b]), objs[b].H, objs[b].W);
}

template <int NSUM, int GATE>
__device__ __forceinline__ void rec_reduce(int* rec, MaskRec<NSUM, GATE> a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) a.sum[k] += __shfl_xor(a.sum[k], o, 64);
        a.r0 = min(a.r0, __shfl_xor(a.r0, o, 64)); a.r1 = max(a.r1, __shfl_xor(a.r1, o, 64));
        a.c0 = min(a.c0, __shfl_xor(a.c0, o, 64)); a.c1 = max(a.c1, __shfl_xor(a.c1, o, 64));
    }
    __shared__ int red[4][NSUM + 4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) red[wave][k] = a.sum[k];
        red[wave][NSUM] = a.r0; red[wave][NSUM + 1] = a.r1; red[wave][NSUM + 2] = a.c0; red[wave][NSUM + 3] = a.c1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
#pragma unroll
            for (int k = 0; k < NSUM; ++k) red[0][k] += red[w][k];
            red[0][NSUM] = min(red[0][NSUM], red[w][NSUM]); red[0][NSUM + 1] = max(red[0][NSUM + 1], red[w][NSUM + 1]);
            red[0][NSUM + 2] = min(red[0][NSUM + 2], red[w][NSUM + 2]); red[0][NSUM + 3] = max(red[0][NSUM + 3], red[w][NSUM + 3]);
        }
#pragma unroll
        for (int k = 0; k < NSUM; ++k)
            if (red[0][k]) atomicAdd(rec + k, red[0][k]);
        if (red[0][GATE]) {
            atomicMin(rec + NSUM, red[0][NSUM]); atomicMax(rec + NSUM + 1, red[0][NSUM + 1]);
            atomicMin(rec + NSUM + 2, red[0][NSUM + 2]); atomicMax(rec + NSUM + 3, red[0][NSUM + 3]);
        }
    }
}

//     roi_value: pixel (r, c) of ZoomIn.inv_transform's canvas: the [S_h, S_w] map src resized to the roi of d (copied when
//     the roi has the map's size; sh, sw: the steps of that resize) and pasted into zeros.
template <class D>
__device__ __forceinline__ float roi_value(const D& d, const float* __restrict__ src, int S_h, int S_w, bool copy, float sh,
                                           float sw, int r, int c) {
    if (r >= d.r0 && r <= d.r1 && c >= d.c0 && c <= d.c1)
        return copy ? src[(int64_t)(r - d.r0) * S_w + (c - d.c0)] : ac_sample(src, S_w, S_h, S_w, sh, sw, r - d.r0, c - d.c0);
    return 0.f;
}

//     The packed mask: pixel i is bit i & 63 of word i >> 6.  With four pixels per lane a wave covers 256 pixels = 4 words per
//     turn k; lanes 16j .. 16j + 15 hold the nibbles of word 4k + j, joined by four xor-shuffles inside the 16-lane group, whose
//     first lane stores the word: every word is written once with a plain store (no atomics, no zero-fill first).  All 64
//     lanes must call it.
__device__ __forceinline__ void quad_word_store(uint64_t* __restrict__ bits, int64_t k, int lane, unsigned nib, int64_t words) {
    unsigned long long word = (unsigned long long)nib << (4 * (lane & 15));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) word |= __shfl_xor(word, o, 64);
    const int64_t at = (k << 2) + (lane >> 4);
    if ((lane & 15) == 0 && at < words) bits[at] = word;
}

//     load4 / store4: the four pixels from i0 on of a flat [HW] map, fp32 (16-byte aligned) or 16-bit labels (8-byte aligned): one
//     access when the quad is whole, else the pixels below HW one by one (the quad that holds the last HW % 4 pixels, or none).
//     The label store writes a whole quad as it stands and, of a partial one, only the pixels whose bit is set in nib.
__device__ __forceinline__ void load4(const float* p, int64_t i0, int64_t HW, float (&v)[4]) {
    if (i0 + 3 < HW) {
        const float4 f = *reinterpret_cast<const float4*>(p + i0);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < HW) v[u] = p[i0 + u];
    }
}

__device__ __forceinline__ void load4(const uint16_t* p, int64_t i0, int64_t HW, unsigned (&v)[4]) {
    if (i0 + 3 < HW) {
        const uint2 q = *reinterpret_cast<const uint2*>(p + i0);
        v[0] = q.x & 0xffffu; v[1] = q.x >> 16; v[2] = q.y & 0xffffu; v[3] = q.y >> 16;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < HW) v[u] = p[i0 + u];
    }
}

__device__ __forceinline__ void load4(const int* p, int64_t i0, int64_t HW, int (&v)[4]) {
    if (i0 + 3 < HW) {
        const int4 q = *reinterpret_cast<const int4*>(p + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < HW) v[u] = p[i0 + u];
    }
}

__device__ __forceinline__ void store4(float* p, int64_t i0, int64_t HW, const float (&v)[4]) {
    if (i0 + 3 < HW) {
        *reinterpret_cast<float4*>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u < HW) p[i0 + u] = v[u];
    }
}

__device__ __forceinline__ void store4(uint16_t* p, int64_t i0, int64_t HW, const unsigned (&v)[4], unsigned nib) {
    if (i0 + 3 < HW) {
        *reinterpret_cast<uint2*>(p + i0) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (nib & (1u << u)) p[i0 + u] = (uint16_t)v[u];
    }
}

// -------------------------------------------------------------------------------------------------------------------
// (1) network input: crop_resize(cat(image, prev), roi, (S_h, S_w)) of object b into batch slot d.src and, with flip, its
//     mirror image into slot n + d.src (AddHorizontalFlip on a batch: [straight..., mirrored...]).  A crop already of the
//     output size is copied, as crop_resize does (it clones instead of resizing).  4 output pixels per thread along a row.
__global__ __launch_bounds__(256) void roi_resize_kernel(const vpu_eval_obj* __restrict__ objs, int n, float* __restrict__ out,
                                                         int S_h, int S_w, int flip, int channels) {
    const vpu_eval_obj& d = objs[blockIdx.y];
    const int h = d.r1 - d.r0 + 1, w = d.c1 - d.c0 + 1;
    const bool copy = h == S_h && w == S_w;
    const float sh = ac_scale(h, S_h), sw = ac_scale(w, S_w);
    const int quads = S_w / 4;                                  // (host: S_w % 4 == 0)
    const int64_t plane = (int64_t)S_h * S_w;
    const int64_t total = (int64_t)channels * S_h * quads;
    float* straight = out + (int64_t)d.src * channels * plane;
    float* mirrored = out + ((int64_t)n + d.src) * channels * plane;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int X = (int)(q % quads) * 4;
        const int Y = (int)((q / quads) % S_h);
        const int c = (int)(q / ((int64_t)quads * S_h));
        const float* src = (c < 3 ? d.image + (int64_t)c * d.H * d.W : d.prev) + (int64_t)d.r0 * d.W + d.c0;
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            v[u] = copy ? src[(int64_t)Y * d.W + X + u] : ac_sample(src, d.W, h, w, sh, sw, Y, X + u);
        const int64_t o = (int64_t)c * plane + (int64_t)Y * S_w;
        *reinterpret_cast<float4*>(straight + o + X) = make_float4(v[0], v[1], v[2], v[3]);
        if (flip) *reinterpret_cast<float4*>(mirrored + o + (S_w - 4 - X)) = make_float4(v[3], v[2], v[1], v[0]);
    }
}

// -------------------------------------------------------------------------------------------------------------------
// (2) ZoomIn.inv_transform + the per-click bookkeeping in one pass over each object's [H, W] canvas: the [S_h, S_w]
//     probability map d.src resized to the roi's (h, w) and pasted into zeros, the mask canvas > pred_thr, the IoU counts
//     of that mask against gt inside valid (utils.get_iou), and the box of canvas > box_thr (vpu_mask_bbox without the
//     clicks: the host joins them, it knows the click of the next step only after this read-back).
//     stats (int32 view of d.out + 2): PasteRec, {intersection, union, count, rmin, rmax, cmin, cmax, 0}.
__device__ __forceinline__ void paste_pixel(const vpu_eval_obj& d, const float* __restrict__ src, int S_h, int S_w, bool copy,
                                            float sh, float sw, float pred_thr, float box_thr, int64_t i, uint8_t g,
                                            uint8_t valid, float& v, uint8_t& m, PasteRec& a) {
    const int r = (int)(i / d.W), c = (int)(i - (int64_t)r * d.W);
    v = roi_value(d, src, S_h, S_w, copy, sh, sw, r, c);
    m = v > pred_thr ? 1 : 0;
    if (valid) {
        a.sum[0] += (m && g) ? 1 : 0;                    // intersection
        a.sum[1] += (m || g) ? 1 : 0;                    // union
    }
    if (v > box_thr) a.count(r, c);
}

__global__ __launch_bounds__(256) void roi_paste_kernel(const vpu_eval_obj* __restrict__ objs, const float* __restrict__ probs,
                                                        int S_h, int S_w, float pred_thr, float box_thr) {
    const vpu_eval_obj& d = objs[blockIdx.y];
    const int h = d.r1 - d.r0 + 1, w = d.c1 - d.c0 + 1;
    const bool copy = h == S_h && w == S_w;
    // the map is resized from (S_h, S_w) to the roi's (h, w): steps of that resize
    const float sh = ac_scale(S_h, h), sw = ac_scale(S_w, w);
    const float* src = probs + (int64_t)d.src * S_h * S_w;
    const int64_t HW = (int64_t)d.H * d.W, quads = HW / 4;
    PasteRec a;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        const uchar4 g = *reinterpret_cast<const uchar4*>(d.gt + 4 * q);
        const uchar4 vl = *reinterpret_cast<const uchar4*>(d.valid + 4 * q);
        float v[4]; uint8_t m[4];
        paste_pixel(d, src, S_h, S_w, copy, sh, sw, pred_thr, box_thr, 4 * q + 0, g.x, vl.x, v[0], m[0], a);
        paste_pixel(d, src, S_h, S_w, copy, sh, sw, pred_thr, box_thr, 4 * q + 1, g.y, vl.y, v[1], m[1], a);
        paste_pixel(d, src, S_h, S_w, copy, sh, sw, pred_thr, box_thr, 4 * q + 2, g.z, vl.z, v[2], m[2], a);
        paste_pixel(d, src, S_h, S_w, copy, sh, sw, pred_thr, box_thr, 4 * q + 3, g.w, vl.w, v[3], m[3], a);
        *reinterpret_cast<float4*>(d.canvas + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<uchar4*>(d.mask + 4 * q) = make_uchar4(m[0], m[1], m[2], m[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(HW - 4 * quads)) {        // the last HW % 4 pixels
        const int64_t i = 4 * quads + threadIdx.x;
        float v; uint8_t m;
        paste_pixel(d, src, S_h, S_w, copy, sh, sw, pred_thr, box_thr, i, d.gt[i], d.valid[i], v, m, a);
        d.canvas[i] = v;
        d.mask[i] = m;
    }
    rec_reduce(rec_of(d), a);
}

// -------------------------------------------------------------------------------------------------------------------
// (3) oracle click keys (Clicker._deepest_errors_device) of every object in one pass per stage.
//     The error masks of object b go to planes 2b (false negatives) and 2b + 1 (false positives) of a [2n][Hm][Wm]
//     canvas, zero beyond the object's own [H, W]; one vpu_edt (zero_border) over all planes; then the masked arg-max
//     over the object's own region with its own not-clicked map and its own raster index r * W + c.
//     Why the zero padding does not change a distance inside [0, H) x [0, W): the reference pads each error mask with a
//     1-pixel zero frame, i.e. rows -1 and H, columns -1 and W.  The padded canvas has those zeros too (its row H /
//     column W, or vpu_edt's own frame when H == Hm / W == Wm), plus further zeros farther out.  Every such extra zero q
//     lies outside the box [-1, H] x [-1, W]; clamping q's coordinates into the box gives a frame pixel that is at least
//     as close to any pixel inside (projection onto a box shortens every distance to points in it).  So the nearest
//     zero is at the same distance with or without the extra zeros.
__global__ __launch_bounds__(256) void click_err_kernel(const vpu_eval_obj* __restrict__ objs, uint8_t* __restrict__ err,
                                                        int Hm, int Wm) {
    const vpu_eval_obj& d = objs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (d.clear_at >= 0) d.keep[d.clear_at] = 0;       // the click just made (Clicker.add_click marks it)
        d.out[0] = 0; d.out[1] = 0;                        // keys: max-reduced below
    }
    const int64_t plane = (int64_t)Hm * Wm, quads = plane / 4;   // (host: Wm % 4 == 0, so a quad lies in one row)
    uint8_t* fn = err + 2 * (int64_t)blockIdx.y * plane;
    uint8_t* fp = fn + plane;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
        const int r = (int)(4 * q / Wm), c = (int)(4 * q - (int64_t)r * Wm);
        uint8_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        if (r < d.H) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c + u < d.W) {
                    const int64_t i = (int64_t)r * d.W + c + u;
                    const bool p = d.mask[i] != 0, g = d.gt[i] != 0, v = d.valid[i] != 0;
                    a[u] = (g && !p && v) ? 1 : 0;
                    b[u] = (!g && p && v) ? 1 : 0;
                }
            }
        }
        *reinterpret_cast<uchar4*>(fn + 4 * q) = make_uchar4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<uchar4*>(fp + 4 * q) = make_uchar4(b[0], b[1], b[2], b[3]);
    }
}

// keys (float bits of max(dist * keep)) << 32 | (0xFFFFFFFF - first raster index): vpu_masked_argmax's packing
__global__ __launch_bounds__(256) void click_argmax_kernel(const vpu_eval_obj* __restrict__ objs, const float* __restrict__ dist,
                                                           int Hm, int Wm) {
    const int b = blockIdx.y >> 1, e = blockIdx.y & 1;
    const vpu_eval_obj& d = objs[b];
    const float* dd = dist + (int64_t)blockIdx.y * Hm * Wm;
    const int HW = d.H * d.W;
    unsigned long long best = 0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const int r = i / d.W, c = i - r * d.W;
        const float v = d.keep[i] ? dd[(int64_t)r * Wm + c] : 0.0f;
        const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (0xFFFFFFFFu - (unsigned)i);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o, 64);
        best = t > best ? t : best;
    }
    __shared__ unsigned long long red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) best = red[k] > best ? red[k] : best;
        atomicMax(reinterpret_cast<unsigned long long*>(d.out) + e, best);
    }
}

// -------------------------------------------------------------------------------------------------------------------
// (4) box prompts of a size group (BasePredictor.get_vqu_prediction, base.py:114-121, then cal_box(as_allmask=False,
//     jitter_box=False)): one row per object and, with flip, one more per object's flip copy.
//     box_masks_kernel: ground truth (1 / 0 / -1 where ignored, the float values the sequential path resizes) and previous
//       prediction sampled over the row's roi to (S_h, S_w) with ac_sample's formula, thresholded to the false-negative
//       (bit 0) and false-positive (bit 1) masks, and their pixel counts.  A flip row reads source column W - 1 - c
//       INSIDE THE UN-MIRRORED roi: the sequential code flips the full planes first and crops them with the same roi.
//     box_choose_kernel: the larger of the two masks (fn when count(fn) > count(fp)), selected on the device.
//     vpu_cc_roots / vpu_cc_table over the R chosen planes, then box_finish_kernel, one block per row.
__device__ __forceinline__ float box_gt_at(const vpu_box_row& d, int r, int c) {
    const int64_t i = (int64_t)r * d.W + (d.mirror ? d.W - 1 - c : c);
    return d.gt[i] ? 1.f : (d.valid[i] ? 0.f : -1.f);
}
__device__ __forceinline__ float box_prev_at(const vpu_box_row& d, int r, int c) {
    return d.prev[(int64_t)r * d.W + (d.mirror ? d.W - 1 - c : c)];
}

__global__ __launch_bounds__(256) void box_masks_kernel(const vpu_box_row* __restrict__ rows, uint8_t* __restrict__ masks,
                                                        int* __restrict__ counts, int S_h, int S_w, float pred_thresh) {
    const vpu_box_row& d = rows[blockIdx.y];
    const int h = d.r1 - d.r0 + 1, w = d.c1 - d.c0 + 1;
    const bool copy = h == S_h && w == S_w;
    const float sh = ac_scale(h, S_h), sw = ac_scale(w, S_w);
    const int total = S_h * S_w;
    uint8_t* out = masks + (int64_t)blockIdx.y * total;
    int nfn = 0, nfp = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int Y = i / S_w, X = i - Y * S_w;
        float g, p;
        if (copy) {
            g = box_gt_at(d, d.r0 + Y, d.c0 + X);
            p = box_prev_at(d, d.r0 + Y, d.c0 + X);
        } else {        // ac_sample (interp_ac.h), the same expression in the same order, on the crop's pixels
            int y0, y1, x0, x1; float ly, lx;
            src_index_ac(Y, sh, h, y0, y1, ly);
            src_index_ac(X, sw, w, x0, x1, lx);
            const float hy = 1.f - ly, hx = 1.f - lx;
            y0 += d.r0; y1 += d.r0; x0 += d.c0; x1 += d.c0;
            g = hy * (hx * box_gt_at(d, y0, x0) + lx * box_gt_at(d, y0, x1)) +
                ly * (hx * box_gt_at(d, y1, x0) + lx * box_gt_at(d, y1, x1));
            p = hy * (hx * box_prev_at(d, y0, x0) + lx * box_prev_at(d, y0, x1)) +
                ly * (hx * box_prev_at(d, y1, x0) + lx * box_prev_at(d, y1, x1));
        }
        const bool gt = g > 0.5f;
        const bool fn = gt && p < pred_thresh, fp = !gt && p > pred_thresh;
        out[i] = (uint8_t)((fn ? 1 : 0) | (fp ? 2 : 0));
        nfn += fn ? 1 : 0;
        nfp += fp ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nfn += __shfl_xor(nfn, o, 64); nfp += __shfl_xor(nfp, o, 64); }
    __shared__ int red[4][2];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = nfn; red[threadIdx.x >> 6][1] = nfp; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (v) atomicAdd(counts + 2 * blockIdx.y + threadIdx.x, v);
    }
}

__global__ __launch_bounds__(256) void box_choose_kernel(uint8_t* __restrict__ masks, const int* __restrict__ counts, int total) {
    const int shift = counts[2 * blockIdx.y] > counts[2 * blockIdx.y + 1] ? 0 : 1;      // cal_box: fn only when strictly larger
    uint8_t* m = masks + (int64_t)blockIdx.y * total;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) m[i] = (m[i] >> shift) & 1;
}

// max_connected_regions (trainer.py:1175-1190; prompt_sim._kept_region_boxes) scans a row's components in ascending root
// (= label) order, tracks the largest so far (first one on ties), re-targets every component with cnt > 0.1 * total onto
// the largest so far and keeps the components whose target is the final largest M.  In closed form, with M the
// component of maximal count and, among those, the smallest root: the largest-so-far at component j is M exactly when
// root_j >= root_M (M is the FIRST to reach the maximum, and nothing after it exceeds it), and a component that is not
// re-targeted keeps its own label, which is M only for M itself.  So kept = {M} + {j : root_j > root_M and
// cnt_j > 0.1 * total}, which needs no sorted table: two order-free block reductions over the rows of vpu_cc_table.
// The comparison is the reference's, in double.
__global__ __launch_bounds__(256) void box_finish_kernel(const vpu_box_row* __restrict__ rows, const float* __restrict__ points,
                                                         const int* __restrict__ counts, const int* __restrict__ table, int kmax,
                                                         int n_batch, int plane, int* __restrict__ boxes, int* __restrict__ flag) {
    const int row = blockIdx.x, wave = threadIdx.x >> 6;
    const int found = table[6 * (int64_t)kmax];
    const int K = found < kmax ? found : kmax;
    if (row == 0 && threadIdx.x == 0) *flag = found > kmax ? 1 : 0;      // table truncated: the host derives this step's boxes
    const int lo = row * plane, hi = lo + plane;           // (host: rows * plane < 2^31)
    __shared__ unsigned long long red_key[4];
    __shared__ long long red_sum[4];
    __shared__ int red_box[4][4];
    unsigned long long best = 0ull;
    long long total = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int root = table[6 * k], cnt = table[6 * k + 1];
        if (root >= lo && root < hi) {
            total += cnt;
            const unsigned long long key = ((unsigned long long)(unsigned)cnt << 32) | (0xFFFFFFFFu - (unsigned)root);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o, 64);
        best = t > best ? t : best;
        total += __shfl_xor(total, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { red_key[wave] = best; red_sum[wave] = total; }
    __syncthreads();
    best = red_key[0]; total = red_sum[0];
    for (int k = 1; k < 4; ++k) { best = red_key[k] > best ? red_key[k] : best; total += red_sum[k]; }
    const int m_root = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    const double tenth = 0.1 * (double)total;
    int y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int* t = table + 6 * k;
        const int root = t[0];
        if (root >= lo && root < hi && (root == m_root || (root > m_root && (double)t[1] > tenth))) {
            y0 = min(y0, t[2]); y1 = max(y1, t[3]); x0 = min(x0, t[4]); x1 = max(x1, t[5]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        y0 = min(y0, __shfl_xor(y0, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
        x0 = min(x0, __shfl_xor(x0, o, 64)); x1 = max(x1, __shfl_xor(x1, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { red_box[wave][0] = y0; red_box[wave][1] = y1; red_box[wave][2] = x0; red_box[wave][3] = x1; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; ++k) {
        y0 = min(y0, red_box[k][0]); y1 = max(y1, red_box[k][1]); x0 = min(x0, red_box[k][2]); x1 = max(x1, red_box[k][3]);
    }
    int out[5] = {0, 0, 0, 0, 0};
    if (best != 0ull) {
        // the slot in the object's own click layout (n_obj rows per polarity) moved into the padded one (n_batch rows):
        // fn: the last positive row n_obj - 1 of both; fp: the first free negative row n_obj + j (default j = n_obj - 1)
        // is row n_batch + j of the padded layout
        const int n_obj = rows[row].n_obj;
        int slot = n_obj - 1;
        if (!(counts[2 * row] > counts[2 * row + 1])) {
            int j = n_obj - 1;
            const float* neg = points + ((int64_t)row * 2 * n_batch + n_batch) * 3;
            for (int q = 0; q < n_obj; ++q)
                if (neg[3 * q + 2] < 0.f) { j = q; break; }
            slot = n_batch + j;
        }
        const int xc = (x0 + x1) >> 1, yc = (y0 + y1) >> 1, bw = x1 - x0, bh = y1 - y0;
        if (xc >= 1 && yc >= 1 && bw >= 1 && bh >= 1) { out[0] = xc; out[1] = yc; out[2] = bw; out[3] = bh; out[4] = slot; }
    }
    for (int k = 0; k < 5; ++k) boxes[5 * row + k] = out[k];
}

// -------------------------------------------------------------------------------------------------------------------
// (5) interactive sessions (isegm/inference/sessions.py): (2)'s canvas without ground truth, plus what the caller of
//     a click wants back: the mask canvas > pred_thr at one bit per pixel, its area, and the ZoomIn box of canvas > box_thr.
//     rec (int32 [8]): SessionRec, {area, count, rmin, rmax, cmin, cmax, 0, 0}.
//     64 consecutive pixels make a word of the packed mask, and a wave has 64 lanes, so every word is produced inside one
//     wave and written once with a plain store (no atomics on the packed buffer, no zero-fill first).
__device__ __forceinline__ float session_pixel(const vpu_session_obj& d, const float* __restrict__ src, int S_h, int S_w, bool copy,
                                               float sh, float sw, float box_thr, int64_t i, SessionRec& a) {
    const int r = (int)(i / d.W), c = (int)(i - (int64_t)r * d.W);
    const float v = roi_value(d, src, S_h, S_w, copy, sh, sw, r, c);
    if (v > box_thr) a.count(r, c);
    return v;
}

// form 0: one pixel per lane; a wave's ballot over its 64 consecutive pixels is the word.  The loop runs over words and its
// bounds depend on the wave only, so all 64 lanes reach the ballot; lanes past H * W vote 0 (the padding bits)
__global__ __launch_bounds__(256) void session_paste_ballot_kernel(const vpu_session_obj* __restrict__ objs,
                                                                   const float* __restrict__ probs, int S_h, int S_w,
                                                                   float pred_thr, float box_thr) {
    const vpu_session_obj& d = objs[blockIdx.y];
    const int h = d.r1 - d.r0 + 1, w = d.c1 - d.c0 + 1;
    const bool copy = h == S_h && w == S_w;
    const float sh = ac_scale(S_h, h), sw = ac_scale(S_w, w);
    const float* src = probs + (int64_t)d.src * S_h * S_w;
    const int64_t HW = (int64_t)d.H * d.W, words = (HW + 63) >> 6;
    const int lane = threadIdx.x & 63;
    SessionRec a;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < words; k += (int64_t)gridDim.x * 4) {
        const int64_t i = (k << 6) + lane;
        bool m = false;
        if (i < HW) {
            const float v = session_pixel(d, src, S_h, S_w, copy, sh, sw, box_thr, i, a);
            d.canvas[i] = v;
            m = v > pred_thr;
            a.sum[0] += m ? 1 : 0;                                    // area
        }
        const unsigned long long word = __ballot(m);
        if (lane == 0) d.bits[k] = word;
    }
    rec_reduce(d.rec, a);
}

// form 1: four pixels per lane (one 16-byte canvas store) and quad_word_store's four words per wave and turn
__global__ __launch_bounds__(256) void session_paste_quad_kernel(const vpu_session_obj* __restrict__ objs,
                                                                 const float* __restrict__ probs, int S_h, int S_w,
                                                                 float pred_thr, float box_thr) {
    const vpu_session_obj& d = objs[blockIdx.y];
    const int h = d.r1 - d.r0 + 1, w = d.c1 - d.c0 + 1;
    const bool copy = h == S_h && w == S_w;
    const float sh = ac_scale(S_h, h), sw = ac_scale(S_w, w);
    const float* src = probs + (int64_t)d.src * S_h * S_w;
    const int64_t HW = (int64_t)d.H * d.W, words = (HW + 63) >> 6, turns = (HW + 255) >> 8;
    const int lane = threadIdx.x & 63;
    SessionRec a;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < turns; k += (int64_t)gridDim.x * 4) {
        const int64_t i0 = (k << 8) + 4 * lane;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned nib = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < HW) {
                v[u] = session_pixel(d, src, S_h, S_w, copy, sh, sw, box_thr, i0 + u, a);
                if (v[u] > pred_thr) { nib |= 1u << u; ++a.sum[0]; }      // area
            }
        }
        store4(d.canvas, i0, HW, v);
        quad_word_store(d.bits, k, lane, nib, words);
    }
    rec_reduce(d.rec, a);
}

// -------------------------------------------------------------------------------------------------------------------
// (6) Crops (pvpuformer_amd/isegm/inference/transforms/crops.py): the network input cut into a grid of overlapping tiles
//     of the trained size, and the tiles' probabilities averaged back.  Both are plain streams, one launch for all tiles.
//
//     gather: tile t = iy * nx + ix (blockIdx.y) = in[:, dy:dy+ch, dx:dx+cw].  4 pixels of a tile row per thread.  The offsets
//     are arbitrary integers and W need not be a multiple of 4, so a source quad is 16-byte aligned only where
//     (c * H + dy + r) * W + dx is a multiple of 4: that holds or fails for a whole tile row at once (the quads of a row
//     start 4 floats apart), and a row takes the 16-byte loads when it holds, scalar loads otherwise.  The destination is
//     dense: 16-byte stores whenever cw % 4 == 0 (vec_out).  A tile whose offsets leave the image is not written.
__global__ __launch_bounds__(256) void crops_gather_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           const int* __restrict__ y_off, const int* __restrict__ x_off, int C,
                                                           int H, int W, int ch, int cw, int nx, int vec_in, int vec_out) {
    const int t = blockIdx.y, dy = y_off[t / nx], dx = x_off[t % nx];
    if (dy < 0 || dx < 0 || dy > H - ch || dx > W - cw) return;
    const int quads = (cw + 3) / 4;
    const int64_t total = (int64_t)C * ch * quads;
    float* dst = out + (int64_t)t * C * ch * cw;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int j = (int)(q % quads) * 4;
        const int r = (int)((q / quads) % ch);
        const int c = (int)(q / ((int64_t)quads * ch));
        const int64_t s = ((int64_t)c * H + dy + r) * W + dx + j;
        const int64_t o = ((int64_t)c * ch + r) * cw + j;
        const int nv = cw - j < 4 ? cw - j : 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (nv == 4 && vec_in && (s & 3) == 0) {
            const float4 f = *reinterpret_cast<const float4*>(in + s);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < nv) v[u] = in[s + u];
        }
        if (nv == 4 && vec_out) {
            *reinterpret_cast<float4*>(dst + o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < nv) dst[o + u] = v[u];
        }
    }
}

//     blend: every output pixel is computed by the lane that owns it -- the covering tiles' values added in tile order (iy
//     ascending, ix ascending inside) to 0, then ONE correctly rounded division by their number: the bits of
//     ``zeros; canvas[tile] += probs[t] for t in order; canvas / counts``.  No atomics, and nothing is read from out.
//     A pixel no tile covers is 0 / 0.
__device__ __forceinline__ float crops_blend_pixel(const float* __restrict__ probs, const int* __restrict__ y_off,
                                                   const int* __restrict__ x_off, int ny, int nx, int ch, int cw, int r, int c) {
    const int64_t plane = (int64_t)ch * cw;
    float acc = 0.f;
    int cover = 0;
    for (int iy = 0; iy < ny; ++iy) {
        const int y = r - y_off[iy];
        if (y < 0 || y >= ch) continue;
        for (int ix = 0; ix < nx; ++ix) {
            const int x = c - x_off[ix];
            if (x < 0 || x >= cw) continue;
            acc += probs[((int64_t)iy * nx + ix) * plane + (int64_t)y * cw + x];
            ++cover;
        }
    }
    return acc / (float)cover;
}

// 4 consecutive pixels of the flat [H * W] map per thread (they may lie in two rows when W % 4 != 0): one 16-byte store
__global__ __launch_bounds__(256) void crops_blend_kernel(const float* __restrict__ probs, float* __restrict__ out,
                                                          const int* __restrict__ y_off, const int* __restrict__ x_off, int ny,
                                                          int nx, int H, int W, int ch, int cw, int vec_out) {
    const int64_t HW = (int64_t)H * W, quads = (HW + 3) >> 2;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < quads; k += (int64_t)gridDim.x * 256) {
        const int64_t i0 = k << 2;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < HW) {
                const int r = (int)((i0 + u) / W), c = (int)((i0 + u) - (int64_t)r * W);
                v[u] = crops_blend_pixel(probs, y_off, x_off, ny, nx, ch, cw, r, c);
            }
        }
        if (vec_out && i0 + 3 < HW) {
            *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u < HW) out[i0 + u] = v[u];
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------
// (7) multi-object annotation (isegm/inference/annotation.py): the object being edited is cur = max(total, add) of two fp32
//     maps (the finished parts and the session's prediction), its mask cur > thr.  One launch composes n annotations of
//     different sizes: the packed mask, rec = AnnotRec, {area, overwritten, rmin, rmax, cmin, cmax, 0, 0}, and by mode
//     total = cur (bit 0) and labels = label where the mask is set (bit 1).  Four pixels per lane: 16-byte loads of both maps,
//     the four labels of a quad in one 8-byte load and, when the mask touches them, one store; the quad is owned by its lane,
//     so the pixels whose bit is clear are written back as they were read.

// the mask pixel (r, c) u places after the quad's first pixel (r0, c0): a quad may span several rows when W < 4
template <class Rec>
__device__ __forceinline__ void annot_count(Rec& a, int r, int c, int W) {
    while (c >= W) { c -= W; ++r; }
    a.count(r, c);
}

__global__ __launch_bounds__(256) void annot_compose_kernel(const vpu_annot_obj* __restrict__ objs, float thr) {
    const vpu_annot_obj& d = objs[blockIdx.y];
    if (d.H < 1 || d.W < 1) return;
    const int64_t HW = (int64_t)d.H * d.W, words = (HW + 63) >> 6, turns = (HW + 255) >> 8;
    const int lane = threadIdx.x & 63;
    const bool put_total = (d.mode & 1) && d.total, put_labels = (d.mode & 2) && d.labels;
    const unsigned label = (unsigned)d.label & 0xffffu;
    AnnotRec a;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < turns; k += (int64_t)gridDim.x * 4) {
        const int64_t i0 = (k << 8) + 4 * lane;
        float t[4] = {0.f, 0.f, 0.f, 0.f}, ad[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned lb[4] = {0u, 0u, 0u, 0u};
        if (d.total) load4(d.total, i0, HW, t);
        if (d.add) load4(d.add, i0, HW, ad);
        if (d.labels) load4(d.labels, i0, HW, lb);
        unsigned nib = 0;
        if (i0 < HW) {
            const int r0 = (int)(i0 / d.W), c0 = (int)(i0 - (int64_t)r0 * d.W);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u < HW) {
                    t[u] = fmaxf(t[u], ad[u]);
                    if (t[u] > thr) {
                        nib |= 1u << u;
                        annot_count(a, r0, c0 + u, d.W);
                        if (lb[u] != 0u && lb[u] != label) ++a.sum[1];        // overwritten
                        lb[u] = label;
                    }
                }
            }
        }
        if (put_total) store4(d.total, i0, HW, t);
        if (put_labels && nib) store4(d.labels, i0, HW, lb, nib);
        quad_word_store(d.bits, k, lane, nib, words);
    }
    rec_reduce(d.rec, a);
}

__global__ void rec_init_one_kernel(int* rec, int H, int W) { rec_init<2>(rec, H, W); }

// out = (labels == label) ? 1 : 0, and those label pixels become 0: the mask a committed object is reopened with; rec: AnnotRec
__global__ __launch_bounds__(256) void label_extract_kernel(uint16_t* __restrict__ labels, float* __restrict__ out,
                                                            int* __restrict__ rec, int H, int W, unsigned label) {
    const int64_t HW = (int64_t)H * W, quads = (HW + 3) >> 2;
    AnnotRec a;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < quads; k += (int64_t)gridDim.x * 256) {
        const int64_t i0 = k << 2;
        unsigned lb[4] = {0u, 0u, 0u, 0u};
        load4(labels, i0, HW, lb);
        const int r0 = (int)(i0 / W), c0 = (int)(i0 - (int64_t)r0 * W);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned nib = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < HW && lb[u] == label) {
                nib |= 1u << u;
                v[u] = 1.f;
                lb[u] = 0u;
                annot_count(a, r0, c0 + u, W);
            }
        }
        store4(out, i0, HW, v);
        if (nib) store4(labels, i0, HW, lb, nib);
    }
    rec_reduce(rec, a);
}

// -------------------------------------------------------------------------------------------------------------------
// (8) run-length maps (isegm/inference/runs.py): the (start, value) pairs of COCO's column-major stream i = c * H + r of n maps
//     of different sizes, v = src > thr (kind 0, fp32) or the 16-bit label (kind 1).  A run starts at i == 0 and wherever
//     v_i != v_{i-1}; the predecessor of (0, c) is (H - 1, c - 1).
//
//     walk: one wave per block; a lane owns a column and walks VPU_RUNS_BAND_ROWS rows of it top to bottom, so a wave's loads
//     are one row segment of VPU_RUNS_COLS values and the stream predecessor of a pixel is the lane's own previous value: no
//     transpose, no LDS, no barrier.  One extra load gives the predecessor of the first row the lane visits.  The count form
//     writes the lane's number of run starts to scratch[item * stride + c * bands + band] (stream order inside an item); the
//     write form starts from the scanned value there and stores one (start, value) per run start, 8 bytes each.
template <int KIND>
__device__ __forceinline__ unsigned runs_value(const void* __restrict__ src, int64_t i, float thr) {
    if (KIND == 0) return reinterpret_cast<const float*>(src)[i] > thr ? 1u : 0u;
    return reinterpret_cast<const uint16_t*>(src)[i];
}

template <int KIND, bool WRITE>
__device__ __forceinline__ void runs_walk(const vpu_runs_obj& d, int c, int r0, int r1, int* __restrict__ slot,
                                          int2* __restrict__ entries, int cap) {
    const int64_t W = d.W;
    const float thr = d.thr;
    // the value no pixel has: the first pixel of the stream always starts a run
    unsigned prev = 0xffffffffu;
    if (r0 > 0) prev = runs_value<KIND>(d.src, (int64_t)(r0 - 1) * W + c, thr);
    else if (c > 0) prev = runs_value<KIND>(d.src, (int64_t)(d.H - 1) * W + c - 1, thr);
    int count = 0;
    unsigned rank = WRITE ? (unsigned)*slot : 0u;
    const int start0 = c * d.H;                                       // (host: H * W < 2^31)
    for (int r = r0; r < r1; r += 8) {
        unsigned v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = r + u < r1 ? runs_value<KIND>(d.src, (int64_t)(r + u) * W + c, thr) : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r + u < r1) {
                if (v[u] != prev) {
                    if (WRITE) {
                        if (rank < (unsigned)cap) entries[rank] = make_int2(start0 + r + u, (int)v[u]);
                        ++rank;
                    } else {
                        ++count;
                    }
                }
                prev = v[u];
            }
        }
    }
    if (!WRITE) *slot = count;
}

template <bool WRITE>
__global__ __launch_bounds__(VPU_RUNS_COLS) void runs_walk_kernel(const vpu_runs_obj* __restrict__ objs, int bands_max,
                                                                  int64_t stride, int* __restrict__ scratch,
                                                                  int2* __restrict__ entries, int cap) {
    const vpu_runs_obj& d = objs[blockIdx.y];
    const int bands = (d.H + VPU_RUNS_BAND_ROWS - 1) / VPU_RUNS_BAND_ROWS;
    const int band = blockIdx.x % bands_max, c = (blockIdx.x / bands_max) * VPU_RUNS_COLS + threadIdx.x;
    if (band >= bands || c >= d.W) return;
    const int r0 = band * VPU_RUNS_BAND_ROWS, r1 = min(r0 + VPU_RUNS_BAND_ROWS, d.H);
    int* slot = scratch + (int64_t)blockIdx.y * stride + (int64_t)c * bands + band;
    if (d.kind == 0) runs_walk<0, WRITE>(d, c, r0, r1, slot, entries, cap);
    else runs_walk<1, WRITE>(d, c, r0, r1, slot, entries, cap);
}

//     scan: ONE workgroup turns the counts of all items into exclusive prefix sums in place, item after item and 4096 entries
//     per turn (four per thread), and writes header[k] = the rank of item k's first run, header[n] = the total.  No workgroup
//     waits on another; the array is W * bands entries per item.
__global__ __launch_bounds__(1024) void runs_scan_kernel(const vpu_runs_obj* __restrict__ objs, int n, int64_t stride,
                                                         int* __restrict__ scratch, int* __restrict__ header) {
    __shared__ int wave_sum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;                                                    // the same value in every thread
    for (int k = 0; k < n; ++k) {
        if (tid == 0) header[k] = carry;
        const int64_t len = (int64_t)objs[k].W * ((objs[k].H + VPU_RUNS_BAND_ROWS - 1) / VPU_RUNS_BAND_ROWS);
        int* base = scratch + (int64_t)k * stride;
        for (int64_t off = 0; off < len; off += 4096) {
            const int64_t i0 = off + 4 * tid;
            int x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = i0 + u < len ? base[i0 + u] : 0;
            const int own = x[0] + x[1] + x[2] + x[3];
            int incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                const int s = wave_sum[w];
                if (w < wave) before += s;
                all += s;
            }
            int at = carry + before + incl - own;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u < len) base[i0 + u] = at;
                at += x[u];
            }
            carry += all;
            __syncthreads();                                          // wave_sum is written again in the next turn
        }
    }
    if (tid == 0) header[n] = carry;
}

// -------------------------------------------------------------------------------------------------------------------
// (9) run-length maps back onto the device: n (start, value) streams, the layout (8) writes, decoded into n maps of different
//     sizes; dst = value == label ? 1.0f : 0.0f (kind 0, fp32) or the value as uint16 (kind 1).
//
//     The mirror of (8)'s walk: one wave per block, a lane owns a column and walks VPU_RUNS_BAND_ROWS rows of it top to bottom,
//     so a wave's stores are one row segment of VPU_RUNS_COLS values.  At its first pixel i0 a lane finds j = the last run whose
//     start <= i0 by a binary search over the start words; from then on it keeps value_j and entry j + 1 in registers and steps
//     when i reaches that start -- at most once per pixel, since starts increase strictly -- with one 8-byte load per step.  No
//     LDS, no barrier, no atomics.
//     Bounds, whatever the entries hold: j stays in 0 .. n_runs - 1 (the search runs over [0, n_runs), the step stops at the
//     last run), so only entries[0 .. n_runs) is read; only (r, c) with r < H, c < W is written, each once.
__device__ __forceinline__ int2 unrun_next(const int2* __restrict__ e, int j, int n_runs) {
    // the entry after run j; beyond the last run a start no pixel reaches (host: H * W < 2^31)
    return j + 1 < n_runs ? e[j + 1] : make_int2(0x7fffffff, 0);
}

template <int KIND>
__device__ __forceinline__ void unrun_walk(const vpu_unrun_obj& d, int c, int r0, int r1) {
    const int2* __restrict__ e = reinterpret_cast<const int2*>(d.entries);
    const int n_runs = d.n_runs, label = d.label;
    const int64_t W = d.W;
    const int start0 = c * d.H;                                       // (host: H * W < 2^31)
    int lo = 0, hi = n_runs;                                          // upper bound of the first pixel over the starts
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (e[mid].x <= start0 + r0) lo = mid + 1;
        else hi = mid;
    }
    int j = max(lo - 1, 0);
    int value = e[j].y;
    int2 next = unrun_next(e, j, n_runs);
    for (int r = r0; r < r1; r += 8) {
        int v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r + u < r1 && start0 + r + u >= next.x) {
                ++j;
                value = next.y;
                next = unrun_next(e, j, n_runs);
            }
            v[u] = value;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (r + u < r1) {
                const int64_t at = (int64_t)(r + u) * W + c;
                if (KIND == 0) reinterpret_cast<float*>(d.dst)[at] = v[u] == label ? 1.0f : 0.0f;
                else reinterpret_cast<uint16_t*>(d.dst)[at] = (uint16_t)v[u];
            }
        }
    }
}

__global__ __launch_bounds__(VPU_RUNS_COLS) void unrun_walk_kernel(const vpu_unrun_obj* __restrict__ objs, int bands_max) {
    const vpu_unrun_obj& d = objs[blockIdx.y];
    const int bands = (d.H + VPU_RUNS_BAND_ROWS - 1) / VPU_RUNS_BAND_ROWS;
    const int band = blockIdx.x % bands_max, c = (blockIdx.x / bands_max) * VPU_RUNS_COLS + threadIdx.x;
    if (band >= bands || c >= d.W) return;
    const int r0 = band * VPU_RUNS_BAND_ROWS, r1 = min(r0 + VPU_RUNS_BAND_ROWS, d.H);
    if (d.kind == 0) unrun_walk<0>(d, c, r0, r1);
    else unrun_walk<1>(d, c, r0, r1);
}

// -------------------------------------------------------------------------------------------------------------------
// (9) region clean-up (isegm/inference/regions.py, rules T1-T8 of include/vpu_hip.h): islands dropped, holes filled, on n
//     maps of different sizes, with no table of components.  Per item the scratch holds a 4-int header (the packed key of the
//     largest component), lab [HW] (the union-find parents: first of the foreground of M, 8-connected, then -- rewritten in
//     place -- of the background of M1, 4-connected, and last of the result M2, 8-connected; -1 off the labelled set), accA [HW] and accB [HW]: area in bits 0 .. 30
//     and one flag in bit 31 (A: holds a positive seed; B: touches the border or holds a negative seed) of the component whose
//     root is that pixel.  Every labelling kernel gives lane l of a wave pixel (block * 256 + thread) of the flat map, so a wave
//     is 64 consecutive pixels at a multiple of 64.  Kernel boundaries order the passes; inside a pass pixels talk only
//     through agent-scope integer atomics (cc_union.h, atomicAdd / Or / Max), which makes the result independent of their order.
constexpr int TIDY_FLAG = (int)0x80000000;

struct TidyItem {
    int64_t HW;
    int *hdr, *lab, *accA, *accB;
    __device__ __forceinline__ explicit TidyItem(const vpu_tidy_obj& d) : HW((int64_t)d.H * d.W), hdr(d.scratch), lab(d.scratch + 4),
                                                                         accA(d.scratch + 4 + HW), accB(d.scratch + 4 + 2 * HW) {}
};

//     The first pixel of the horizontal run of lane's pixel inside its wave (-1 off the set): a run starts where the lane
//     below is off the set, at lane 0 and at column 0.  The pieces of a run that spans waves are joined by tidy_merge_kernel.
//     All 64 lanes must call it.
__device__ __forceinline__ int tidy_run_start(bool member, bool row_start, int i, int lane) {
    const unsigned long long on = __builtin_amdgcn_ballot_w64(member), rs = __builtin_amdgcn_ballot_w64(row_start);
    const unsigned long long starts = on & (~(on << 1) | rs | 1ull);
    if (!member) return -1;
    const unsigned long long below = starts & ((2ull << lane) - 1ull);      // (not empty: the run's lowest lane is a start)
    return i - (lane - (63 - __builtin_clzll(below)));
}

//     acc[r] += 1 (OR false) or acc[r] |= TIDY_FLAG (OR true) for the lanes that are on: one atomic per wave when they all have
//     the same root (Guideline 12; the common case, a wave inside one region), one per lane otherwise.  All 64 lanes must call it.
template <bool OR>
__device__ __forceinline__ void tidy_wave_acc(int* __restrict__ acc, int r, bool on, int lane) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(on);
    if (mask == 0) return;
    const int first = __builtin_ctzll(mask), r0 = __shfl(r, first, 64);
    const bool uniform = __builtin_amdgcn_ballot_w64(on && r != r0) == 0;
    if (uniform) {
        if (lane == first) {
            if (OR) atomicOr(acc + r0, TIDY_FLAG);
            else atomicAdd(acc + r0, __builtin_popcountll(mask));
        }
    } else if (on) {
        if (OR) atomicOr(acc + r, TIDY_FLAG);
        else atomicAdd(acc + r, 1);
    }
}

#define TIDY_PIXEL                                                                        \
    const vpu_tidy_obj& d = objs[blockIdx.y];                                             \
    const TidyItem s(d);                                                                  \
    if ((int64_t)blockIdx.x * 256 >= s.HW) return;                                        \
    const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;                          \
    const bool in = i64 < s.HW;                                                           \
    const int i = (int)i64, lane = threadIdx.x & 63

//     M = max(total, add) > thr: the run starts of its foreground, both accumulators and the header cleared
__global__ __launch_bounds__(256) void tidy_init_kernel(const vpu_tidy_obj* __restrict__ objs, float thr) {
    TIDY_PIXEL;
    bool fg = false;
    if (in) {
        const float t = d.total ? d.total[i] : 0.f, a = d.add ? d.add[i] : 0.f;
        fg = fmaxf(t, a) > thr;
        s.accA[i] = 0;
        s.accB[i] = 0;
    }
    const int v = tidy_run_start(fg, in && i % d.W == 0, i, lane);
    if (in) s.lab[i] = v;
    if (i64 < 4) s.hdr[i] = 0;
}

//     Runs of adjacent rows joined: N / NW / NE for the 8-connected foreground (cc_merge_kernel's rule: a run of the row above
//     is joined once per run of this row), N only for the 4-connected background; and W at lane 0, where tidy_run_start cut.
//     Membership is lab >= 0, which no union changes.
template <bool CONN8>
__global__ __launch_bounds__(256) void tidy_merge_kernel(const vpu_tidy_obj* __restrict__ objs) {
    TIDY_PIXEL;
    int* lab = s.lab;
    if (!in || lab[i] < 0) return;
    const int W = d.W, r = i / W, c = i - r * W;
    const bool left = c > 0 && lab[i - 1] >= 0;
    if (left && lane == 0) cc_union(lab, i, i - 1);
    if (r == 0) return;
    const bool n = lab[i - W] >= 0, nw = c > 0 && lab[i - W - 1] >= 0;
    if (n && !(left && nw)) cc_union(lab, i, i - W);
    if (CONN8) {
        if (!n && nw && !left) cc_union(lab, i, i - W - 1);
        if (!n && c + 1 < W && lab[i - W + 1] >= 0) cc_union(lab, i, i - W + 1);
    }
}

//     lab = the root; the area of every component summed at its root; PHASE 1 (background): the flag of every component that
//     holds a pixel of the first or last row or column
template <int PHASE>
__global__ __launch_bounds__(256) void tidy_flatten_kernel(const vpu_tidy_obj* __restrict__ objs) {
    TIDY_PIXEL;
    int* lab = s.lab;
    const bool on = in && lab[i] >= 0;
    int root = -1;
    if (on) {
        // a read-only walk (the unions are complete): cc_find's path halving would re-point OTHER pixels to a grandparent and
        // could so overwrite the root their own thread has just stored; a walk that meets such a stored root is simply done
        root = i;
        while (true) {
            const int p = __hip_atomic_load(lab + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p == root) break;
            root = p;
        }
        __hip_atomic_store(lab + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int* acc = PHASE == 0 ? s.accA : s.accB;
    tidy_wave_acc<false>(acc, root, on, lane);
    if (PHASE == 1) {
        const int r = i / d.W, c = i - r * d.W;
        tidy_wave_acc<true>(acc, root, on && (r == 0 || r == d.H - 1 || c == 0 || c == d.W - 1), lane);
    }
}

//     the flag of the components that hold a seed: PHASE 0 the positive ones on the foreground, PHASE 1 the negative ones on the
//     background; one block per item
template <int PHASE>
__global__ __launch_bounds__(256) void tidy_seed_kernel(const vpu_tidy_obj* __restrict__ objs) {
    const vpu_tidy_obj& d = objs[blockIdx.x];
    const TidyItem s(d);
    int* acc = PHASE == 0 ? s.accA : s.accB;
    for (int k = threadIdx.x; k < d.n_seeds; k += 256) {
        const int r = d.seeds[3 * k], c = d.seeds[3 * k + 1];
        const bool positive = d.seeds[3 * k + 2] != 0;
        if (r < 0 || r >= d.H || c < 0 || c >= d.W || positive != (PHASE == 0)) continue;
        const int root = s.lab[(int64_t)r * d.W + c];
        if (root >= 0) atomicOr(acc + root, TIDY_FLAG);
    }
}

//     hdr[0 .. 1] = the largest (area, ~root) of the foreground components, vpu_masked_argmax's packing: the greatest area, of equal
//     ones the smallest root; the wave's maximum first, then one atomic per wave
__global__ __launch_bounds__(256) void tidy_largest_kernel(const vpu_tidy_obj* __restrict__ objs) {
    TIDY_PIXEL;
    if (d.keep != VPU_TIDY_LARGEST) return;
    unsigned long long key = 0;
    if (in && s.lab[i] == i) key = ((unsigned long long)(unsigned)(s.accA[i] & ~TIDY_FLAG) << 32) | (unsigned)~i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if (lane == 0 && key) atomicMax(reinterpret_cast<unsigned long long*>(s.hdr), key);
}

//     T2-T4: a pixel is in M1 when its component is kept.  Then lab is rewritten in place -- a thread reads and writes its own
//     entry only -- as the run starts of the background of M1 (-1 on M1).
__global__ __launch_bounds__(256) void tidy_keep_kernel(const vpu_tidy_obj* __restrict__ objs) {
    TIDY_PIXEL;
    bool kept = false;
    if (in && s.lab[i] >= 0) {
        const int root = s.lab[i], a = s.accA[root], area = a & ~TIDY_FLAG;
        kept = a < 0;                                                            // T2: protected by a positive seed
        if (d.keep == VPU_TIDY_ALL) kept = kept || area >= d.min_area;
        if (d.keep == VPU_TIDY_LARGEST) {
            const unsigned long long best = *reinterpret_cast<const unsigned long long*>(s.hdr);
            kept = kept || (best != 0 && (unsigned)root == ~(unsigned)best);
        }
    }
    const int v = tidy_run_start(in && !kept, in && i % d.W == 0, i, lane);
    if (in) s.lab[i] = v;
}

//     T5-T6: lab < 0 is M1; else accB at the pixel's root says whether its background region is a hole that is filled.  lab is
//     rewritten in place once more, as the run starts of M2 (-1 off it): tidy_merge_kernel<true> then labels the result, whose
//     roots are its components (a filled hole joins the ring around it with a kept island inside it).
__global__ __launch_bounds__(256) void tidy_fill_kernel(const vpu_tidy_obj* __restrict__ objs) {
    TIDY_PIXEL;
    bool m2 = false;
    if (in) {
        const int root = s.lab[i];
        m2 = root < 0;
        if (!m2 && d.max_hole > 0) {
            const int hole = s.accB[root];                    // (negative: the region is no hole, or holds a negative seed)
            m2 = hole >= 0 && hole <= d.max_hole;
        }
    }
    const int v = tidy_run_start(m2, in && i % d.W == 0, i, lane);
    if (in) s.lab[i] = v;
}

//     T7-T8 in annot_compose_kernel's quad pattern.  lab >= 0 is M2, and a pixel that is its own parent is the root of one of
//     its components: they are counted into rec[7], the wave's sum first.  The maps are copied with the two edits, M2 packed
//     and counted.
__global__ __launch_bounds__(256) void tidy_apply_kernel(const vpu_tidy_obj* __restrict__ objs, float thr) {
    const vpu_tidy_obj& d = objs[blockIdx.y];
    const TidyItem s(d);
    const int64_t HW = s.HW, words = (HW + 63) >> 6, turns = (HW + 255) >> 8;
    const int lane = threadIdx.x & 63;
    TidyRec a;
    int roots = 0;
    for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < turns; k += (int64_t)gridDim.x * 4) {
        const int64_t i0 = (k << 8) + 4 * lane;
        float t[4] = {0.f, 0.f, 0.f, 0.f}, ad[4] = {0.f, 0.f, 0.f, 0.f};
        int lb[4] = {-1, -1, -1, -1};
        if (d.total) load4(d.total, i0, HW, t);
        if (d.add) load4(d.add, i0, HW, ad);
        load4(s.lab, i0, HW, lb);
        unsigned nib = 0;
        if (i0 < HW) {
            const int r0 = (int)(i0 / d.W), c0 = (int)(i0 - (int64_t)r0 * d.W);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u < HW) {
                    const bool m = fmaxf(t[u], ad[u]) > thr;
                    const bool m2 = lb[u] >= 0;
                    if (lb[u] == (int)(i0 + u)) ++roots;
                    if (m2) {
                        nib |= 1u << u;
                        annot_count(a, r0, c0 + u, d.W);
                    }
                    if (m && !m2) { ++a.sum[1]; t[u] = 0.f; ad[u] = 0.f; }
                    if (m2 && !m) { ++a.sum[2]; t[u] = 1.f; ad[u] = 1.f; }
                }
            }
        }
        if (d.total_out) store4(d.total_out, i0, HW, t);
        if (d.add_out) store4(d.add_out, i0, HW, ad);
        quad_word_store(d.bits, k, lane, nib, words);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) roots += __shfl_xor(roots, o, 64);
    if (lane == 0 && roots) atomicAdd(d.rec + 7, roots);
    rec_reduce(d.rec, a);
}

}  // namespace

static bool crops_sizes_ok(int32_t ny, int32_t nx, int32_t H, int32_t W, int32_t ch, int32_t cw) {
    return ny >= 1 && nx >= 1 && ny <= VPU_CROPS_MAX_TILES_AXIS && nx <= VPU_CROPS_MAX_TILES_AXIS && ch >= 1 && cw >= 1 &&
           ch <= H && cw <= W;
}

extern "C" int vpu_crops_gather(const float* in, float* out, const int32_t* y_offsets, const int32_t* x_offsets, int32_t ny,
                                int32_t nx, int32_t C, int32_t H, int32_t W, int32_t ch, int32_t cw, void* stream) {
    vpu_clear_stale_error();
    if (!in || !out || !y_offsets || !x_offsets || C < 1 || !crops_sizes_ok(ny, nx, H, W, ch, cw)) {
        vpu_set_error("crops_gather: null pointer or sizes (1 <= ny, nx <= VPU_CROPS_MAX_TILES_AXIS, 1 <= ch <= H, 1 <= cw <= W)");
        return VPU_ERR_ARG;
    }
    const int vec_in = reinterpret_cast<uintptr_t>(in) % 16 == 0;
    const int vec_out = cw % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int nb = vpu_grid_for((long long)C * ch * ((cw + 3) / 4), 256, 256);
    crops_gather_kernel<<<dim3((unsigned)nb, (unsigned)(ny * nx)), 256, 0, ST>>>(in, out, y_offsets, x_offsets, C, H, W, ch, cw,
                                                                                nx, vec_in, vec_out);
    return vpu_check_launch("vpu_crops_gather");
}

extern "C" int vpu_crops_blend(const float* probs, float* out, const int32_t* y_offsets, const int32_t* x_offsets, int32_t ny,
                               int32_t nx, int32_t H, int32_t W, int32_t ch, int32_t cw, void* stream) {
    vpu_clear_stale_error();
    if (!probs || !out || !y_offsets || !x_offsets || !crops_sizes_ok(ny, nx, H, W, ch, cw)) {
        vpu_set_error("crops_blend: null pointer or sizes (1 <= ny, nx <= VPU_CROPS_MAX_TILES_AXIS, 1 <= ch <= H, 1 <= cw <= W)");
        return VPU_ERR_ARG;
    }
    const int vec_out = reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int nb = vpu_grid_for(((long long)H * W + 3) / 4, 256, 4096);
    crops_blend_kernel<<<(unsigned)nb, 256, 0, ST>>>(probs, out, y_offsets, x_offsets, ny, nx, H, W, ch, cw, vec_out);
    return vpu_check_launch("vpu_crops_blend");
}

extern "C" int vpu_session_paste_batched(const vpu_session_obj* objs, int32_t n, const float* probs, int32_t S_h, int32_t S_w,
                                         float pred_thr, float box_thr, int32_t max_hw, int32_t form, void* stream) {
    vpu_clear_stale_error();
    if (!objs || !probs || n < 1 || n > 65535 || S_h < 1 || S_w < 1 || max_hw < 1 || (form != 0 && form != 1)) {
        vpu_set_error("session_paste_batched: sizes (1 <= n <= 65535) or form (0: ballot, 1: quads)");
        return VPU_ERR_ARG;
    }
    rec_init_kernel<2><<<(n + 63) / 64, 64, 0, ST>>>(objs, n);
    const int nb = vpu_grid_for(max_hw, 1024, 128);
    if (form == 0)
        session_paste_ballot_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, probs, S_h, S_w, pred_thr, box_thr);
    else
        session_paste_quad_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, probs, S_h, S_w, pred_thr, box_thr);
    return vpu_check_launch("vpu_session_paste_batched");
}

extern "C" int vpu_box_prompts_batched(const vpu_box_row* rows, int32_t n_rows, const float* points, int32_t n_batch, int32_t S_h,
                                       int32_t S_w, float pred_thresh, uint8_t* masks, int32_t* counts, int32_t* roots,
                                       int32_t* slots, int32_t* table, int32_t kmax, int32_t* boxes, int32_t* flag, void* stream) {
    vpu_clear_stale_error();
    const int64_t total = (int64_t)n_rows * S_h * S_w;
    if (!rows || !points || !masks || !counts || !roots || !slots || !table || !boxes || !flag || n_rows < 1 || n_rows > 65535 ||
        n_batch < 1 || S_h < 1 || S_w < 1 || kmax < 1 || total >= 0x7FFFFFFFLL) {
        vpu_set_error("box_prompts_batched: null pointer or sizes (1 <= n_rows <= 65535, n_rows * S_h * S_w < 2^31)");
        return VPU_ERR_ARG;
    }
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t) * n_rows, ST) != hipSuccess) {
        vpu_set_error("box_prompts_batched: memset");
        return VPU_ERR_LAUNCH;
    }
    const int nb = vpu_grid_for((long long)S_h * S_w, 256, 128);
    box_masks_kernel<<<dim3((unsigned)nb, (unsigned)n_rows), 256, 0, ST>>>(rows, masks, counts, S_h, S_w, pred_thresh);
    box_choose_kernel<<<dim3((unsigned)nb, (unsigned)n_rows), 256, 0, ST>>>(masks, counts, S_h * S_w);
    int rc = vpu_check_launch("vpu_box_prompts_batched (masks)");
    if (rc) return rc;
    rc = vpu_cc_roots(masks, roots, n_rows, S_h, S_w, stream);
    if (rc) return rc;
    rc = vpu_cc_table(roots, slots, table, kmax, n_rows, S_h, S_w, stream);
    if (rc) return rc;
    vpu_clear_stale_error();
    box_finish_kernel<<<(unsigned)n_rows, 256, 0, ST>>>(rows, points, counts, table, kmax, n_batch, S_h * S_w, boxes, flag);
    return vpu_check_launch("vpu_box_prompts_batched (boxes)");
}

extern "C" int vpu_roi_resize_batched(const vpu_eval_obj* objs, int32_t n, float* out, int32_t S_h, int32_t S_w, int32_t flip,
                                      int32_t channels, void* stream) {
    vpu_clear_stale_error();
    if (!objs || !out || n < 1 || n > 65535 || S_h < 1 || S_w < 4 || S_w % 4 || (channels != 3 && channels != 4)) {
        vpu_set_error("roi_resize_batched: sizes (1 <= n <= 65535, S_w a multiple of 4, 3 or 4 channels)");
        return VPU_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(out) % 16) { vpu_set_error("roi_resize_batched: out not 16-byte aligned"); return VPU_ERR_ALIGN; }
    const int nb = vpu_grid_for((long long)channels * S_h * (S_w / 4), 256, 256);
    roi_resize_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, n, out, S_h, S_w, flip, channels);
    return vpu_check_launch("vpu_roi_resize_batched");
}

extern "C" int vpu_roi_paste_batched(const vpu_eval_obj* objs, int32_t n, const float* probs, int32_t S_h, int32_t S_w,
                                     float pred_thr, float box_thr, int32_t max_hw, void* stream) {
    vpu_clear_stale_error();
    if (!objs || !probs || n < 1 || n > 65535 || S_h < 1 || S_w < 1 || max_hw < 1) {
        vpu_set_error("roi_paste_batched: sizes (1 <= n <= 65535)");
        return VPU_ERR_ARG;
    }
    rec_init_kernel<3><<<(n + 63) / 64, 64, 0, ST>>>(objs, n);
    const int nb = vpu_grid_for(((long long)max_hw + 3) / 4, 256, 128);
    roi_paste_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, probs, S_h, S_w, pred_thr, box_thr);
    return vpu_check_launch("vpu_roi_paste_batched");
}

extern "C" int vpu_click_keys_batched(const vpu_eval_obj* objs, int32_t n, uint8_t* err, int32_t* scratch, float* dist,
                                      int32_t Hm, int32_t Wm, int32_t max_hw, void* stream) {
    vpu_clear_stale_error();
    if (!objs || !err || !scratch || !dist || n < 1 || n > 32767 || Hm < 1 || Wm < 4 || Wm % 4 || max_hw < 1) {
        vpu_set_error("click_keys_batched: sizes (1 <= n <= 32767, Wm a multiple of 4)");
        return VPU_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(err) % 4) { vpu_set_error("click_keys_batched: err not 4-byte aligned"); return VPU_ERR_ALIGN; }
    const int nb = vpu_grid_for((long long)Hm * Wm / 4, 256, 128);
    click_err_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, err, Hm, Wm);
    int rc = vpu_check_launch("vpu_click_keys_batched (error masks)");
    if (rc) return rc;
    rc = vpu_edt(err, scratch, dist, 2 * n, Hm, Wm, 1, stream);
    if (rc) return rc;
    vpu_clear_stale_error();
    const int na = vpu_grid_for(max_hw, 2048, 128);
    click_argmax_kernel<<<dim3((unsigned)na, (unsigned)(2 * n)), 256, 0, ST>>>(objs, dist, Hm, Wm);
    return vpu_check_launch("vpu_click_keys_batched (arg-max)");
}

extern "C" int vpu_annot_compose_batched(const vpu_annot_obj* objs, int32_t n, float thr, int32_t max_hw, void* stream) {
    vpu_clear_stale_error();
    if (!objs || n < 1 || n > 65535 || max_hw < 1 || !(thr == thr)) {
        vpu_set_error("annot_compose_batched: null descriptors, sizes (1 <= n <= 65535, max_hw >= 1) or a NaN threshold");
        return VPU_ERR_ARG;
    }
    rec_init_kernel<2><<<(n + 63) / 64, 64, 0, ST>>>(objs, n);
    const int nb = vpu_grid_for(max_hw, 1024, 128);
    annot_compose_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, thr);
    return vpu_check_launch("vpu_annot_compose_batched");
}

extern "C" int vpu_label_extract(uint16_t* labels, float* out, int32_t* rec, int32_t H, int32_t W, int32_t label, void* stream) {
    vpu_clear_stale_error();
    if (!labels || !out || !rec || H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff || label < 1 || label > 65535) {
        vpu_set_error("label_extract: null pointer, sizes (H, W >= 1, H * W < 2^31) or label (1 <= label <= 65535)");
        return VPU_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(labels) % 8 || reinterpret_cast<uintptr_t>(out) % 16 || reinterpret_cast<uintptr_t>(rec) % 4) {
        vpu_set_error("label_extract: labels not 8-byte, out not 16-byte or rec not 4-byte aligned");
        return VPU_ERR_ALIGN;
    }
    rec_init_one_kernel<<<1, 1, 0, ST>>>(rec, H, W);
    const int nb = vpu_grid_for(((long long)H * W + 3) / 4, 256, 1024);
    label_extract_kernel<<<(unsigned)nb, 256, 0, ST>>>(labels, out, rec, H, W, (unsigned)label);
    return vpu_check_launch("vpu_label_extract");
}

extern "C" int vpu_regions_tidy_batched(const vpu_tidy_obj* objs, const vpu_tidy_obj* host_objs, int32_t n, float thr, void* stream) {
    vpu_clear_stale_error();
    char msg[256];
    if (!objs || !host_objs || n < 1 || n > 65535 || !(thr >= 0.f && thr < 1.f)) {
        vpu_set_error("regions_tidy_batched: null descriptors, n (1 <= n <= 65535) or thr (0 <= thr < 1)");
        return VPU_ERR_ARG;
    }
    int64_t max_hw = 0;
    bool seeds = false, largest = false;
    for (int32_t k = 0; k < n; ++k) {
        const vpu_tidy_obj& d = host_objs[k];
        if (d.H < 1 || d.W < 1 || (int64_t)d.H * d.W > 0x7fffffffLL || !d.bits || !d.rec || !d.scratch ||
            (!d.add && !d.total && (d.add_out || d.total_out)) || d.n_seeds < 0 || (d.n_seeds > 0 && !d.seeds) || d.min_area < 0 ||
            d.max_hole < 0 || d.keep < VPU_TIDY_ALL || d.keep > VPU_TIDY_LARGEST) {
            snprintf(msg, sizeof msg, "regions_tidy_batched: item %d: sizes (H, W >= 1, H * W < 2^31), a null bits, rec or scratch, an "
                     "output map without an input, seeds, min_area or max_hole < 0, or keep (0: all, 1: seeded, 2: largest)", k);
            vpu_set_error(msg);
            return VPU_ERR_ARG;
        }
        const uintptr_t maps = reinterpret_cast<uintptr_t>(d.add) | reinterpret_cast<uintptr_t>(d.total) |
                               reinterpret_cast<uintptr_t>(d.add_out) | reinterpret_cast<uintptr_t>(d.total_out) |
                               reinterpret_cast<uintptr_t>(d.scratch);
        if (maps % 16 || reinterpret_cast<uintptr_t>(d.bits) % 8 || reinterpret_cast<uintptr_t>(d.rec) % 4 ||
            reinterpret_cast<uintptr_t>(d.seeds) % 4) {
            snprintf(msg, sizeof msg, "regions_tidy_batched: item %d: a map or scratch not 16-byte, bits not 8-byte, rec or seeds not "
                     "4-byte aligned", k);
            vpu_set_error(msg);
            return VPU_ERR_ALIGN;
        }
        const int64_t hw = (int64_t)d.H * d.W;
        max_hw = hw > max_hw ? hw : max_hw;
        seeds = seeds || d.n_seeds > 0;
        largest = largest || d.keep == VPU_TIDY_LARGEST;
    }
    const dim3 pixels((unsigned)((max_hw + 255) / 256), (unsigned)n);
    rec_init_kernel<3><<<(n + 63) / 64, 64, 0, ST>>>(objs, n);
    tidy_init_kernel<<<pixels, 256, 0, ST>>>(objs, thr);
    tidy_merge_kernel<true><<<pixels, 256, 0, ST>>>(objs);
    tidy_flatten_kernel<0><<<pixels, 256, 0, ST>>>(objs);
    if (seeds) tidy_seed_kernel<0><<<(unsigned)n, 256, 0, ST>>>(objs);
    if (largest) tidy_largest_kernel<<<pixels, 256, 0, ST>>>(objs);
    tidy_keep_kernel<<<pixels, 256, 0, ST>>>(objs);
    tidy_merge_kernel<false><<<pixels, 256, 0, ST>>>(objs);
    tidy_flatten_kernel<1><<<pixels, 256, 0, ST>>>(objs);
    if (seeds) tidy_seed_kernel<1><<<(unsigned)n, 256, 0, ST>>>(objs);
    tidy_fill_kernel<<<pixels, 256, 0, ST>>>(objs);
    tidy_merge_kernel<true><<<pixels, 256, 0, ST>>>(objs);
    const int nb = vpu_grid_for(max_hw, 1024, 128);
    tidy_apply_kernel<<<dim3((unsigned)nb, (unsigned)n), 256, 0, ST>>>(objs, thr);
    return vpu_check_launch("vpu_regions_tidy_batched");
}

// The launch geometry of (8) from the host's copy of the descriptors, after every check of them: bands_max and cols_max
// size the grid, stride = the largest W * bands is the distance of two items in scratch.
struct RunsPlan {
    int bands_max = 0, groups_max = 0;
    int64_t stride = 0;
};

static int runs_plan(const char* who, const vpu_runs_obj* objs, const vpu_runs_obj* host_objs, int32_t n, RunsPlan& p) {
    char msg[192];
    if (!objs || !host_objs || n < 1 || n > 65535) {
        snprintf(msg, sizeof msg, "%s: null descriptors or n (1 <= n <= 65535)", who);
        vpu_set_error(msg);
        return VPU_ERR_ARG;
    }
    int64_t pixels = 0;
    for (int32_t k = 0; k < n; ++k) {
        const vpu_runs_obj& d = host_objs[k];
        if (!d.src || d.H < 1 || d.W < 1 || (int64_t)d.H * d.W > 0x7fffffffLL || (d.kind != 0 && d.kind != 1)) {
            snprintf(msg, sizeof msg, "%s: item %d: null src, sizes (H, W >= 1, H * W < 2^31) or kind (0: fp32 > thr, 1: labels)", who, k);
            vpu_set_error(msg);
            return VPU_ERR_ARG;
        }
        if (reinterpret_cast<uintptr_t>(d.src) % (d.kind == 0 ? 16 : 8)) {
            snprintf(msg, sizeof msg, "%s: item %d: src not %d-byte aligned", who, k, d.kind == 0 ? 16 : 8);
            vpu_set_error(msg);
            return VPU_ERR_ALIGN;
        }
        const int bands = (d.H + VPU_RUNS_BAND_ROWS - 1) / VPU_RUNS_BAND_ROWS;
        const int groups = (d.W + VPU_RUNS_COLS - 1) / VPU_RUNS_COLS;
        p.bands_max = bands > p.bands_max ? bands : p.bands_max;
        p.groups_max = groups > p.groups_max ? groups : p.groups_max;
        p.stride = (int64_t)d.W * bands > p.stride ? (int64_t)d.W * bands : p.stride;
        pixels += (int64_t)d.H * d.W;
    }
    // every rank and every scratch index fits an int32, and so does the grid
    if (pixels > 0x7fffffffLL || p.stride * n > 0x7fffffffLL || (int64_t)p.bands_max * p.groups_max > 0x7fffffffLL) {
        snprintf(msg, sizeof msg, "%s: the items together have 2^31 pixels or more", who);
        vpu_set_error(msg);
        return VPU_ERR_ARG;
    }
    return 0;
}

extern "C" int vpu_runs_count_batched(const vpu_runs_obj* objs, const vpu_runs_obj* host_objs, int32_t n, int32_t* scratch,
                                      int64_t scratch_len, int32_t* header, void* stream) {
    vpu_clear_stale_error();
    RunsPlan p;
    const int rc = runs_plan("runs_count_batched", objs, host_objs, n, p);
    if (rc) return rc;
    if (!scratch || !header || scratch_len < p.stride * n) {
        vpu_set_error("runs_count_batched: null scratch or header, or scratch_len below n * max(W * bands)");
        return VPU_ERR_ARG;
    }
    runs_walk_kernel<false><<<dim3((unsigned)(p.bands_max * p.groups_max), (unsigned)n), VPU_RUNS_COLS, 0, ST>>>(
        objs, p.bands_max, p.stride, scratch, nullptr, 0);
    runs_scan_kernel<<<1, 1024, 0, ST>>>(objs, n, p.stride, scratch, header);
    return vpu_check_launch("vpu_runs_count_batched");
}

extern "C" int vpu_runs_write_batched(const vpu_runs_obj* objs, const vpu_runs_obj* host_objs, int32_t n, const int32_t* scratch,
                                      int64_t scratch_len, int32_t* entries, int32_t cap, void* stream) {
    vpu_clear_stale_error();
    RunsPlan p;
    const int rc = runs_plan("runs_write_batched", objs, host_objs, n, p);
    if (rc) return rc;
    if (!scratch || scratch_len < p.stride * n || cap < 0 || (cap > 0 && !entries)) {
        vpu_set_error("runs_write_batched: null scratch or entries, scratch_len below n * max(W * bands), or cap < 0");
        return VPU_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(entries) % 8) { vpu_set_error("runs_write_batched: entries not 8-byte aligned"); return VPU_ERR_ALIGN; }
    runs_walk_kernel<true><<<dim3((unsigned)(p.bands_max * p.groups_max), (unsigned)n), VPU_RUNS_COLS, 0, ST>>>(
        objs, p.bands_max, p.stride, const_cast<int32_t*>(scratch), reinterpret_cast<int2*>(entries), cap);
    return vpu_check_launch("vpu_runs_write_batched");
}

extern "C" int vpu_runs_decode_batched(const vpu_unrun_obj* objs, const vpu_unrun_obj* host_objs, int32_t n, void* stream) {
    vpu_clear_stale_error();
    char msg[224];
    if (!objs || !host_objs || n < 1 || n > 65535) {
        vpu_set_error("runs_decode_batched: null descriptors or n (1 <= n <= 65535)");
        return VPU_ERR_ARG;
    }
    int bands_max = 0, groups_max = 0;
    for (int32_t k = 0; k < n; ++k) {
        const vpu_unrun_obj& d = host_objs[k];
        if (!d.dst || !d.entries || d.H < 1 || d.W < 1 || (int64_t)d.H * d.W > 0x7fffffffLL || d.n_runs < 1 ||
            d.n_runs > (int64_t)d.H * d.W || (d.kind != 0 && d.kind != 1) || (d.kind == 0 && (d.label < 0 || d.label > 65535))) {
            snprintf(msg, sizeof msg, "runs_decode_batched: item %d: null dst or entries, sizes (H, W >= 1, H * W < 2^31), n_runs "
                     "(1 <= n_runs <= H * W), kind (0: fp32 of value == label, 1: labels) or label (0 <= label <= 65535)", k);
            vpu_set_error(msg);
            return VPU_ERR_ARG;
        }
        if (reinterpret_cast<uintptr_t>(d.dst) % (d.kind == 0 ? 16 : 8) || reinterpret_cast<uintptr_t>(d.entries) % 8) {
            snprintf(msg, sizeof msg, "runs_decode_batched: item %d: dst not %d-byte or entries not 8-byte aligned", k, d.kind == 0 ? 16 : 8);
            vpu_set_error(msg);
            return VPU_ERR_ALIGN;
        }
        const int bands = (d.H + VPU_RUNS_BAND_ROWS - 1) / VPU_RUNS_BAND_ROWS;
        const int groups = (d.W + VPU_RUNS_COLS - 1) / VPU_RUNS_COLS;
        bands_max = bands > bands_max ? bands : bands_max;
        groups_max = groups > groups_max ? groups : groups_max;
    }
    if ((int64_t)bands_max * groups_max > 0x7fffffffLL) {
        vpu_set_error("runs_decode_batched: the largest item's bands x column groups do not fit the grid");
        return VPU_ERR_ARG;
    }
    unrun_walk_kernel<<<dim3((unsigned)(bands_max * groups_max), (unsigned)n), VPU_RUNS_COLS, 0, ST>>>(objs, bands_max);
    return vpu_check_launch("vpu_runs_decode_batched");
}
