// Outlines (pvpuformer_amd/isegm/inference/outlines.py): the polygon loops of n binary maps of different
// sizes, rules O1-O6 of include/vpu_hip.h.  Every kernel reads a device array of vpu_outline_obj, so one launch covers all items;
// the grid is sized by the largest item and a block beyond its item returns at once.  Kernels neither allocate nor synchronise,
// no workgroup waits on another, and no launch reads an entry that another thread of the same launch writes.
//
// Corners need no walking.  The 2 x 2 neighbourhood of a lattice vertex (bits NW = 1, NE = 2, SW = 4, SE = 8) decides them: one
// or three pixels set give one corner, a saddle (6 or 9) two, anything else none.  A corner has its rank R in row-major order
// (y, x; at a saddle the corner whose horizontal edge lies to the West first) and its rank C in column-major order (x, y; at a
// saddle the corner whose vertical edge lies to the North first).  Consecutive R on a lattice row are the ends of one horizontal
// edge and consecutive C on a lattice column those of one vertical edge, so the successor of a corner is R + 1 (it leaves East),
// R - 1 (West), the corner of column rank C + 1 (South) or C - 1 (North).
#include <cstdio>

#include "vpu_common.h"
#include "../../include/vpu_hip.h"

#define ST reinterpret_cast<hipStream_t>(stream)

namespace {

// neighbourhoods with a corner, with two, and the leave direction (0 East, 1 South, 2 West, 3 North; two bits per neighbourhood)
// of the corner that comes first in row-major order; the second corner of a saddle leaves the opposite way (dir ^ 2).
//   1 NW: W   2 NE: N   4 SW: S   8 SE: E   7 (SE clear): S   11 (SW clear): W   13 (NE clear): E   14 (NW clear): N
//   9 (NW, SE): W then E   6 (NE, SW): N then S
constexpr unsigned OUT_TWO = (1u << 6) | (1u << 9);
constexpr unsigned OUT_ANY = OUT_TWO | (1u << 1) | (1u << 2) | (1u << 4) | (1u << 8) | (1u << 7) | (1u << 11) | (1u << 13) | (1u << 14);
constexpr unsigned long long OUT_DIRS = (2ull << 2) | (3ull << 4) | (1ull << 8) | (0ull << 16) | (1ull << 14) | (2ull << 22) |
                                        (0ull << 26) | (3ull << 28) | (2ull << 18) | (3ull << 12);

// work int32 [16 V + 2] (16-byte aligned): two ping-pong state arrays of int4 {next, min, dist, -}, then per corner (x, y),
// (dir, C), the table C -> R, the successor, the loop index and the loop offset, then {L, -}.
struct OutlineWork {
    int4 *a, *b;
    int2 *pts, *dc;
    int *tab, *succ, *lidx, *loff, *tot;
};

__host__ __device__ inline OutlineWork outline_work(int32_t* work, int64_t V) {
    OutlineWork w;
    w.a = reinterpret_cast<int4*>(work);
    w.b = reinterpret_cast<int4*>(work + 4 * V);
    w.pts = reinterpret_cast<int2*>(work + 8 * V);
    w.dc = reinterpret_cast<int2*>(work + 10 * V);
    w.tab = work + 12 * V;
    w.succ = work + 13 * V;
    w.lidx = work + 14 * V;
    w.loff = work + 15 * V;
    w.tot = work + 16 * V;
    return w;
}

__host__ __device__ inline int outline_groups(int W) { return (W + VPU_OUTLINE_COLS) / VPU_OUTLINE_COLS; }         // ceil((W + 1) / COLS)
__host__ __device__ inline int outline_bands(int H) { return (H + VPU_OUTLINE_BAND_ROWS) / VPU_OUTLINE_BAND_ROWS; }

// -------------------------------------------------------------------------------------------------------------------
// (1) walk: one wave per block; lane l owns lattice column x = 64 g + l and walks VPU_OUTLINE_BAND_ROWS lattice rows top to
//     bottom, eight loads in flight.  The vertex (x, y) needs the pixels (y - 1, x - 1), (y - 1, x), (y, x - 1), (y, x): the lane
//     loads (y, x), keeps the row above in registers and takes the western pair from lane l - 1 by a shuffle; lane 0 loads its
//     western pixel itself.  So a map value is read once, plus one column per wave and one row per band.  Pixels outside the
//     image are clear; lanes beyond x = W stay in the loop (their neighbourhood is clear) for the shuffles and ballots.
//     The count form writes the corners of (row y, group g) to scratch[item * rs + y * groups + g] (row-major order) and the
//     lane's corners to scratch[n * rs + item * cs + x * bands + band] (column-major order).  The write form starts from the
//     scanned values there, takes the rank inside the row from two ballots, and stores (x, y) and (dir, C) at R and R at C.
template <int KIND>
__device__ __forceinline__ unsigned outline_px(const vpu_outline_obj& d, int r, int c) {
    const int64_t i = (int64_t)r * d.W + c;
    if (KIND == 0) return reinterpret_cast<const float*>(d.src)[i] > d.thr ? 1u : 0u;
    return reinterpret_cast<const uint16_t*>(d.src)[i] == (uint16_t)d.label ? 1u : 0u;
}

template <int KIND, bool WRITE>
__device__ __forceinline__ void outline_walk(const vpu_outline_obj& d, int x, int y0, int y1, int lane, int* __restrict__ rowslot,
                                             int groups, int* __restrict__ colslot, const OutlineWork& w, unsigned V) {
    const int H = d.H, W = d.W;
    const bool own = x < W, west = lane == 0 && x > 0 && x <= W;
    unsigned up = 0, upw = 0;                                         // the pixel row above the lattice row: (y - 1, x), (y - 1, x - 1)
    if (y0 > 0) {
        up = own ? outline_px<KIND>(d, y0 - 1, x) : 0u;
        const unsigned mine = west ? outline_px<KIND>(d, y0 - 1, x - 1) : 0u;
        upw = __shfl_up(up, 1, 64);
        if (lane == 0) upw = mine;
    }
    int count = 0;
    unsigned C = WRITE && x <= W ? (unsigned)*colslot : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int y = y0; y < y1; y += 8) {
        unsigned v[8], vw[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool row = y + u < y1 && y + u < H;
            v[u] = row && own ? outline_px<KIND>(d, y + u, x) : 0u;
            vw[u] = row && west ? outline_px<KIND>(d, y + u, x - 1) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (y + u < y1) {                                         // (the same in every lane)
                unsigned sw = __shfl_up(v[u], 1, 64);
                if (lane == 0) sw = vw[u];
                const unsigned cfg = upw | (up << 1) | (sw << 2) | (v[u] << 3);
                const unsigned any = (OUT_ANY >> cfg) & 1u, two = (OUT_TWO >> cfg) & 1u;
                const unsigned long long b1 = __ballot(any), b2 = __ballot(two);
                if (!WRITE) {
                    if (lane == 0) rowslot[(int64_t)(y + u) * groups] = __popcll(b1) + __popcll(b2);
                    count += any + two;
                } else if (any) {
                    const unsigned R = (unsigned)rowslot[(int64_t)(y + u) * groups] + __popcll(b1 & below) + __popcll(b2 & below);
                    const int dir = (int)((OUT_DIRS >> (2 * cfg)) & 3ull);
                    const unsigned c0 = C + (cfg == 9u ? 1u : 0u);
                    if (R < V && c0 < V) {
                        w.pts[R] = make_int2(x, y + u);
                        w.dc[R] = make_int2(dir, (int)c0);
                        w.tab[c0] = (int)R;
                    }
                    if (two) {
                        const unsigned c1 = C + (cfg == 6u ? 1u : 0u);
                        if (R + 1 < V && c1 < V) {
                            w.pts[R + 1] = make_int2(x, y + u);
                            w.dc[R + 1] = make_int2(dir ^ 2, (int)c1);
                            w.tab[c1] = (int)(R + 1);
                        }
                    }
                    C += 1u + two;
                }
                up = v[u];
                upw = sw;
            }
        }
    }
    if (!WRITE && x <= W) *colslot = count;
}

template <bool WRITE>
__global__ __launch_bounds__(VPU_OUTLINE_COLS) void outline_walk_kernel(const vpu_outline_obj* __restrict__ objs, int n, int bands_max,
                                                                        int64_t rs, int64_t cs, int* __restrict__ scratch,
                                                                        int32_t* __restrict__ work, int V) {
    const int k = blockIdx.y;
    const vpu_outline_obj& d = objs[k];
    const int groups = outline_groups(d.W), bands = outline_bands(d.H);
    const int band = blockIdx.x % bands_max, g = blockIdx.x / bands_max, lane = threadIdx.x;
    if (band >= bands || g >= groups) return;
    const int x = g * VPU_OUTLINE_COLS + lane;
    const int y0 = band * VPU_OUTLINE_BAND_ROWS, y1 = min(y0 + VPU_OUTLINE_BAND_ROWS, d.H + 1);
    int* rowslot = scratch + (int64_t)k * rs + g;
    int* colslot = scratch + (int64_t)n * rs + (int64_t)k * cs + (int64_t)min(x, d.W) * bands + band;
    const OutlineWork w = outline_work(work, V);
    if (d.kind == 0) outline_walk<0, WRITE>(d, x, y0, y1, lane, rowslot, groups, colslot, w, (unsigned)V);
    else outline_walk<1, WRITE>(d, x, y0, y1, lane, rowslot, groups, colslot, w, (unsigned)V);
}

// -------------------------------------------------------------------------------------------------------------------
// (2) scans, the pattern of runs_scan_kernel (evalbatch.hip, section 8): ONE workgroup of 1024 threads per array, 4096 entries
//     per turn (four per thread, a shuffle scan per wave, the 16 wave sums through LDS); no look-back, no flags.
//     block_scan: the exclusive prefix of `own` over the block and the block's total.  Two barriers; wave_sum may be written
//     again after the second.
__device__ __forceinline__ int block_scan(int own, int* wave_sum, int& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const int s = wave_sum[w];
        if (w < wave) before += s;
        all += s;
    }
    __syncthreads();
    return before + incl - own;
}

//     Block 0 turns the row-major counts of all items into exclusive prefix sums in place, item after item, and writes the
//     header; block 1 does the same for the column-major counts.  Both count every corner once, so item k owns the ranks
//     header[k] .. header[k + 1] - 1 in both orders.
__global__ __launch_bounds__(1024) void outline_scan_kernel(const vpu_outline_obj* __restrict__ objs, int n, int64_t rs, int64_t cs,
                                                            int* __restrict__ scratch, int* __restrict__ header) {
    __shared__ int wave_sum[16];
    const int tid = threadIdx.x;
    const bool rows = blockIdx.x == 0;
    int carry = 0;                                                    // the same value in every thread
    for (int k = 0; k < n; ++k) {
        if (rows && tid == 0) header[k] = carry;
        const int64_t len = rows ? (int64_t)(objs[k].H + 1) * outline_groups(objs[k].W) : (int64_t)(objs[k].W + 1) * outline_bands(objs[k].H);
        int* base = scratch + (rows ? (int64_t)k * rs : (int64_t)n * rs + (int64_t)k * cs);
        for (int64_t off = 0; off < len; off += 4096) {
            const int64_t i0 = off + 4 * tid;
            int x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = i0 + u < len ? base[i0 + u] : 0;
            int all;
            int at = carry + block_scan(x[0] + x[1] + x[2] + x[3], wave_sum, all);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + u < len) base[i0 + u] = at;
                at += x[u];
            }
            carry += all;
        }
    }
    if (rows && tid == 0) header[n] = carry;
}

// -------------------------------------------------------------------------------------------------------------------
// (3) link: the successor of every corner, and the first state of the doubling {next = successor, min = R, dist = 0}.  An index
//     that the tables do not bear out (they always do after a count of the same maps) falls back to the corner itself, so that
//     every later index stays inside [0, V) whatever the buffers hold.
__global__ __launch_bounds__(256) void outline_link_kernel(int32_t* __restrict__ work, int V) {
    const OutlineWork w = outline_work(work, V);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const int2 dc = w.dc[i];
    int s;
    if (dc.x == 0) s = i + 1;
    else if (dc.x == 2) s = i - 1;
    else {
        const int c = dc.x == 1 ? dc.y + 1 : dc.y - 1;
        s = (unsigned)c < (unsigned)V ? w.tab[c] : i;
    }
    if ((unsigned)s >= (unsigned)V) s = i;
    w.succ[i] = s;
    w.a[i] = make_int4(s, i, 0, 0);
}

// (4) order: pointer doubling over the closed loops.  After round r a corner knows, for the 2^(r + 1) corners from itself on in
//     the order of travel, the smallest R among them and the number of steps to its first occurrence.  Once the window is as long
//     as the loop, min is the loop's leader (its corner of smallest (y, x)) and dist the steps from the corner to the leader,
//     which gives its position in the loop: the running minimum and the ranking in the same rounds.  A round reads one buffer
//     and writes the other.
__global__ __launch_bounds__(256) void outline_double_kernel(const int4* __restrict__ in, int4* __restrict__ out, int V, int step) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const int4 a = in[i];
    const int4 b = in[a.x];
    out[i] = b.y < a.y ? make_int4(b.x, b.y, step + b.z, 0) : make_int4(b.x, a.y, a.z, 0);
}

//     The loop index is the rank of a leader among the leaders in R order (O4's order, item after item), the loop offset the
//     exclusive sum of the loop lengths in that order; the length of the leader's loop is one more than the distance of its
//     successor.  ONE workgroup, as in (2).
__global__ __launch_bounds__(1024) void outline_loops_kernel(const int4* __restrict__ st, int32_t* __restrict__ work, int V) {
    __shared__ int wave_sum[16];
    const OutlineWork w = outline_work(work, V);
    const int tid = threadIdx.x;
    int loops = 0, corners = 0;                                       // the same values in every thread
    for (int off = 0; off < V; off += 4096) {
        const int i0 = off + 4 * tid;
        int lead[4], len[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u;
            lead[u] = i < V && st[i].y == i ? 1 : 0;
            len[u] = lead[u] ? st[w.succ[i]].z + 1 : 0;
        }
        int all_loops, all_len;
        int at_loop = loops + block_scan(lead[0] + lead[1] + lead[2] + lead[3], wave_sum, all_loops);
        int at_len = corners + block_scan(len[0] + len[1] + len[2] + len[3], wave_sum, all_len);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < V) {
                w.lidx[i0 + u] = at_loop;
                w.loff[i0 + u] = at_len;
            }
            at_loop += lead[u];
            at_len += len[u];
        }
        loops += all_loops;
        corners += all_len;
    }
    if (tid == 0) w.tot[0] = loops;
}

// (5) place: every corner stores its (x, y) with one 8-byte store at offset[loop] + position, every leader its loop's offset;
//     the first n + 1 threads write the items' first loops, thread 0 the closing offset.  Only entries below the caps are written.
__global__ __launch_bounds__(256) void outline_place_kernel(const int4* __restrict__ st, const int32_t* __restrict__ work, int V, int n,
                                                            const int* __restrict__ header, int2* __restrict__ points, int cap,
                                                            int* __restrict__ offsets, int loop_cap, int* __restrict__ item_loops) {
    const OutlineWork w = outline_work(const_cast<int32_t*>(work), V);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n) {
        const int h = header[i], total = w.tot[0];
        item_loops[i] = (unsigned)h < (unsigned)V ? w.lidx[h] : total;
        if (i == 0 && (unsigned)total < (unsigned)loop_cap) offsets[total] = V;
    }
    if (i >= V) return;
    const int4 s = st[i];
    const int leader = s.y;
    const int len = st[w.succ[leader]].z + 1;
    const int at = w.loff[leader] + (s.z == 0 ? 0 : len - s.z);
    if ((unsigned)at < (unsigned)cap) points[at] = w.pts[i];
    if (leader == i && (unsigned)w.lidx[i] < (unsigned)loop_cap) offsets[w.lidx[i]] = w.loff[i];
}

// The launch geometry from the host's copy of the descriptors, after every check of them.
struct OutlinePlan {
    int bands_max = 0, groups_max = 0;
    int64_t rs = 0, cs = 0;                                           // the largest (H + 1) * groups and (W + 1) * bands
};

int outline_plan(const char* who, const vpu_outline_obj* objs, const vpu_outline_obj* host_objs, int32_t n, OutlinePlan& p) {
    char msg[256];
    if (!objs || !host_objs || n < 1 || n > 65535) {
        snprintf(msg, sizeof msg, "%s: null descriptors or n (1 <= n <= 65535)", who);
        vpu_set_error(msg);
        return VPU_ERR_ARG;
    }
    int64_t slots = 0;
    for (int32_t k = 0; k < n; ++k) {
        const vpu_outline_obj& d = host_objs[k];
        const bool kind_ok = d.kind == 0 ? d.thr >= 0.0f && d.thr < 1.0f : d.kind == 1 && d.label >= 0 && d.label <= 65535;
        if (!d.src || d.H < 1 || d.W < 1 || !kind_ok) {
            snprintf(msg, sizeof msg, "%s: item %d: null src, sizes (H, W >= 1), kind (0: fp32 > thr with 0 <= thr < 1, 1: labels "
                     "== label with 0 <= label <= 65535)", who, k);
            vpu_set_error(msg);
            return VPU_ERR_ARG;
        }
        if (reinterpret_cast<uintptr_t>(d.src) % (d.kind == 0 ? 16 : 8)) {
            snprintf(msg, sizeof msg, "%s: item %d: src not %d-byte aligned", who, k, d.kind == 0 ? 16 : 8);
            vpu_set_error(msg);
            return VPU_ERR_ALIGN;
        }
        slots += 2 * ((int64_t)d.H + 1) * ((int64_t)d.W + 1);
        if (slots > 0x7fffffffLL) {                                   // every rank and every lattice index fits an int32
            snprintf(msg, sizeof msg, "%s: the items together have 2^30 lattice vertices or more", who);
            vpu_set_error(msg);
            return VPU_ERR_ARG;
        }
        const int bands = outline_bands(d.H), groups = outline_groups(d.W);
        p.bands_max = bands > p.bands_max ? bands : p.bands_max;
        p.groups_max = groups > p.groups_max ? groups : p.groups_max;
        const int64_t rs = ((int64_t)d.H + 1) * groups, cs = ((int64_t)d.W + 1) * bands;
        p.rs = rs > p.rs ? rs : p.rs;
        p.cs = cs > p.cs ? cs : p.cs;
    }
    if ((int64_t)p.bands_max * p.groups_max > 0x7fffffffLL) {
        snprintf(msg, sizeof msg, "%s: the largest item's bands x column groups do not fit the grid", who);
        vpu_set_error(msg);
        return VPU_ERR_ARG;
    }
    return 0;
}

}  // namespace

extern "C" int vpu_outline_count_batched(const vpu_outline_obj* objs, const vpu_outline_obj* host_objs, int32_t n, int32_t* scratch,
                                         int64_t scratch_len, int32_t* header, void* stream) {
    vpu_clear_stale_error();
    OutlinePlan p;
    const int rc = outline_plan("outline_count_batched", objs, host_objs, n, p);
    if (rc) return rc;
    if (!scratch || !header || scratch_len < (p.rs + p.cs) * n) {
        vpu_set_error("outline_count_batched: null scratch or header, or scratch_len below n * (max((H + 1) * groups) + max((W + 1) * bands))");
        return VPU_ERR_ARG;
    }
    outline_walk_kernel<false><<<dim3((unsigned)(p.bands_max * p.groups_max), (unsigned)n), VPU_OUTLINE_COLS, 0, ST>>>(
        objs, n, p.bands_max, p.rs, p.cs, scratch, nullptr, 0);
    outline_scan_kernel<<<2, 1024, 0, ST>>>(objs, n, p.rs, p.cs, scratch, header);
    return vpu_check_launch("vpu_outline_count_batched");
}

extern "C" int vpu_outline_trace_batched(const vpu_outline_obj* objs, const vpu_outline_obj* host_objs, int32_t n, const int32_t* scratch,
                                         int64_t scratch_len, const int32_t* header, const int32_t* host_header, int32_t* work,
                                         int64_t work_len, int32_t* points, int32_t cap, int32_t* offsets, int32_t loop_cap,
                                         int32_t* item_loops, void* stream) {
    vpu_clear_stale_error();
    OutlinePlan p;
    const int rc = outline_plan("outline_trace_batched", objs, host_objs, n, p);
    if (rc) return rc;
    if (!scratch || scratch_len < (p.rs + p.cs) * n || !header || !host_header || cap < 0 || loop_cap < 0 || (cap > 0 && !points) ||
        (loop_cap > 0 && !offsets) || !item_loops) {
        vpu_set_error("outline_trace_batched: null scratch, header, host_header, points, offsets or item_loops, scratch_len below "
                      "n * (max((H + 1) * groups) + max((W + 1) * bands)), or a negative cap");
        return VPU_ERR_ARG;
    }
    int most = 0;
    bool ok = host_header[0] == 0;
    for (int32_t k = 0; ok && k < n; ++k) {                           // what a count of these items can have left
        const int64_t v = (int64_t)host_header[k + 1] - host_header[k];
        ok = v >= 0 && v <= 2 * ((int64_t)host_objs[k].H + 1) * ((int64_t)host_objs[k].W + 1);
        most = v > most ? (int)v : most;
    }
    if (!ok) {
        vpu_set_error("outline_trace_batched: host_header is not the header of a count of these items");
        return VPU_ERR_ARG;
    }
    const int V = host_header[n];
    if (V > 0 && (!work || work_len < VPU_OUTLINE_WORK_INTS(V))) {
        vpu_set_error("outline_trace_batched: null work or work_len below VPU_OUTLINE_WORK_INTS(V)");
        return VPU_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(work) % 16 || reinterpret_cast<uintptr_t>(points) % 8 || reinterpret_cast<uintptr_t>(offsets) % 8) {
        vpu_set_error("outline_trace_batched: work not 16-byte or points or offsets not 8-byte aligned");
        return VPU_ERR_ALIGN;
    }
    if (V == 0) return 0;                                             // no corner anywhere: nothing to launch
    const OutlineWork w = outline_work(work, V);
    const unsigned per_corner = (unsigned)((V + 255) / 256);
    outline_walk_kernel<true><<<dim3((unsigned)(p.bands_max * p.groups_max), (unsigned)n), VPU_OUTLINE_COLS, 0, ST>>>(
        objs, n, p.bands_max, p.rs, p.cs, const_cast<int32_t*>(scratch), work, V);
    outline_link_kernel<<<per_corner, 256, 0, ST>>>(work, V);
    int4 *from = w.a, *to = w.b;
    for (int64_t step = 1; step < most; step <<= 1) {                     // ceil(log2(the most corners of an item)) rounds
        outline_double_kernel<<<per_corner, 256, 0, ST>>>(from, to, V, (int)step);
        int4* t = from; from = to; to = t;
    }
    outline_loops_kernel<<<1, 1024, 0, ST>>>(from, work, V);
    const int64_t threads = V > n + 1 ? V : n + 1;
    outline_place_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, ST>>>(from, work, V, n, header, reinterpret_cast<int2*>(points), cap,
                                                                            offsets, loop_cap, item_loops);
    return vpu_check_launch("vpu_outline_trace_batched");
}

// ===================================================================================================================
// Simplified polygons (pvpuformer_amd/isegm/inference/polygons.py): Douglas-Peucker, rules S1-S6 of
// include/vpu_hip.h, over the loops the trace left on the device.  Workgroups do not communicate: no grid barrier, and no
// workgroup reads what another one of the same launch writes.
//
// Rounds instead of recursion.  Every position that is not kept and whose chain may still split knows its chain (i, j), the kept
// positions around it.  A round finds each chain's k of largest num (the smallest k on ties) and applies S4; a chain that does
// not split never will, so its positions retire.  After a split every position of the chain compares itself with k and takes
// (i, k) or (k, j): no scan is needed to find the new chain ends.  S3 is the first round: S4 on the chain (0, n), whose ends are
// both P_0, with t = 0.  The kept set does not depend on the order of the splits, so it is the sequential one.
namespace {

// work int32 [10 V + 5 Lm + 8] (16-byte aligned), Lm = loop_max: the largest num of the chain that begins at a position, in two
// copies that the rounds use in turn (int64), the smallest position that has it (two copies), per position its chain (i, j) or
// {-1, next kept} once kept or {-2, -} once retired, its rank among the kept of its loop (-1: not kept) and its loop; per loop
// the kept count (0: dropped), the hole flag, the rounds, and the exclusive sums of surviving loops and kept points.
struct SimplifyWork {
    long long* best;
    int *bpos, *rank, *loopof, *cnt, *lhole, *rounds, *nidx, *noff;
    int2* state;
};

__host__ __device__ inline SimplifyWork simplify_work(int32_t* work, int64_t V, int64_t Lm) {
    SimplifyWork w;
    w.best = reinterpret_cast<long long*>(work);                      // [2][V]
    w.state = reinterpret_cast<int2*>(work + 4 * V);                  // [V]
    w.bpos = work + 6 * V;                                            // [2][V]
    w.rank = work + 8 * V;
    w.loopof = work + 9 * V;
    w.cnt = work + 10 * V;
    w.lhole = w.cnt + Lm;
    w.rounds = w.lhole + Lm;
    w.nidx = w.rounds + Lm;                                           // [Lm + 1]
    w.noff = w.nidx + Lm + 1;                                         // [Lm + 1]
    return w;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the loop l of the trace's output with every index clamped: its first corner and its length
__device__ __forceinline__ void simplify_loop(const int* __restrict__ offsets, int l, int V, int& a, int& n) {
    a = clampi(offsets[l], 0, V);
    n = clampi(offsets[l + 1], a, V) - a;
}

// S2: the squared distance of P to the segment A B as num / den.  Coordinates lie in 0 .. 8191 (S1), so a difference is below
// 2^13, a squared length, a dot and a cross product below 2^27, num below 2^54 and the two sides of S4, 16 num and t^2 den with
// t <= 2^12, below 2^58 and 2^51: exact in int64.
__device__ __forceinline__ void simplify_distance(int px, int py, int ax, int ay, int bx, int by, long long& num, long long& den) {
    const int ux = bx - ax, uy = by - ay, vx = px - ax, vy = py - ay, wx = px - bx, wy = py - by;
    const long long da = (long long)(vx * vx + vy * vy), db = (long long)(wx * wx + wy * wy);
    const long long d = (long long)(ux * ux + uy * uy), dot = (long long)(vx * ux + vy * uy), cross = (long long)(ux * vy - uy * vx);
    den = d == 0 ? 1 : d;
    num = d == 0 ? da : (dot <= 0 ? da * d : (dot >= d ? db * d : cross * cross));
}

__device__ __forceinline__ long long cross2(int2 p, int2 q) { return (long long)(p.x * q.y - q.x * p.y); }      // below 2^27

__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

#define SIMPLIFY_WAVES (VPU_SIMPLIFY_THREADS / 64)

// -------------------------------------------------------------------------------------------------------------------
// (1) split, form A: one workgroup per loop, any length, its positions block-strided.  A round has three steps with a barrier
//     after each: every live position adds its num to its chain's maximum (the slot of the chain's first position i; an integer
//     atomic maximum, exact and order-free); every live position that has the maximum offers its position to the chain's minimum;
//     every live position reads (num, k) of its chain, applies S4 and takes its new chain, and position k clears the slot pair
//     that the next round uses at i.  The slots are read with atomic loads: they were written by atomics, which the CU's vector
//     L1 does not see.  The block-wide OR of the splits ends the rounds, at most n of them: a round that splits keeps a vertex.
__global__ __launch_bounds__(VPU_SIMPLIFY_THREADS) void simplify_split_a_kernel(const int2* __restrict__ points, const int* __restrict__ offsets,
                                                                                const int* __restrict__ item_loops, int n_items, int V,
                                                                                int loop_max, int t, int skip_short, int32_t* __restrict__ work) {
    __shared__ long long red[2][SIMPLIFY_WAVES];
    __shared__ int wave_cnt[SIMPLIFY_WAVES];
    const SimplifyWork w = simplify_work(work, V, loop_max);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = clampi(item_loops[n_items], 0, loop_max);
    for (int l = blockIdx.x; l < L; l += gridDim.x) {
        int a, n;
        simplify_loop(offsets, l, V, a, n);
        if (skip_short && n <= VPU_SIMPLIFY_SHORT) continue;          // (the same in every thread)
        const int2* __restrict__ P = points + a;
        int2* state = w.state + a;
        long long* best[2] = {w.best + a, w.best + V + a};
        int* bpos[2] = {w.bpos + a, w.bpos + V + a};
        for (int p = tid; p < n; p += VPU_SIMPLIFY_THREADS) {
            state[p] = p == 0 ? make_int2(-1, n) : make_int2(0, n);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                __hip_atomic_store(best[s] + p, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(bpos[s] + p, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        int rounds = 0;
        long long tt = 0;                                             // S3: the first round is S4 with t = 0
        for (int r = 0; r <= n; ++r) {
            long long* bst = best[r & 1];
            int* bps = bpos[r & 1];
            for (int p = tid; p < n; p += VPU_SIMPLIFY_THREADS) {
                const int2 s = state[p];
                if (s.x < 0) continue;
                const int i = clampi(s.x, 0, n - 1), j = clampi(s.y, 1, n);
                const int2 pp = P[p], pa = P[i], pb = P[j == n ? 0 : j];
                long long num, den;
                simplify_distance(pp.x, pp.y, pa.x, pa.y, pb.x, pb.y, num, den);
                __hip_atomic_fetch_max(bst + i, num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            for (int p = tid; p < n; p += VPU_SIMPLIFY_THREADS) {
                const int2 s = state[p];
                if (s.x < 0) continue;
                const int i = clampi(s.x, 0, n - 1), j = clampi(s.y, 1, n);
                const int2 pp = P[p], pa = P[i], pb = P[j == n ? 0 : j];
                long long num, den;
                simplify_distance(pp.x, pp.y, pa.x, pa.y, pb.x, pb.y, num, den);
                if (num == __hip_atomic_load(bst + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    __hip_atomic_fetch_min(bps + i, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            int any = 0;
            for (int p = tid; p < n; p += VPU_SIMPLIFY_THREADS) {
                const int2 s = state[p];
                if (s.x < 0) continue;
                const int i = clampi(s.x, 0, n - 1), j = clampi(s.y, 1, n);
                const int2 pa = P[i], pb = P[j == n ? 0 : j];
                const int ux = pb.x - pa.x, uy = pb.y - pa.y;
                const long long d = (long long)(ux * ux + uy * uy), den = d == 0 ? 1 : d;
                const long long num = __hip_atomic_load(bst + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int k = clampi(__hip_atomic_load(bps + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0, n - 1);
                if (16 * num > tt * den) {                            // S4; both sides below 2^58 (simplify_distance)
                    any = 1;
                    if (p < k) state[p] = make_int2(i, k);
                    else if (p > k) state[p] = make_int2(k, j);
                    else {
                        state[p] = make_int2(-1, j);                  // kept: its successor among the kept, and i's
                        state[i].y = k;                               // (position i is kept: its own thread leaves it alone)
                        __hip_atomic_store(best[(r + 1) & 1] + i, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(bpos[(r + 1) & 1] + i, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else {
                    state[p] = make_int2(-2, 0);
                }
            }
            if (!__syncthreads_or(any)) break;
            ++rounds;
            tt = (long long)t * t;
        }
        // the kept positions' ranks, the kept count, and twice the signed areas of the exact and of the simplified loop (S5)
        int carry = 0;
        long long exact = 0, simple = 0;
        for (int base = 0; base < n; base += VPU_SIMPLIFY_THREADS) {
            const int p = base + tid;
            int kept = 0;
            if (p < n) {
                const int2 s = state[p], pp = P[p];
                kept = s.x == -1 ? 1 : 0;
                exact += cross2(pp, P[p + 1 < n ? p + 1 : 0]);
                if (kept) {
                    const int q = clampi(s.y, 1, n);
                    simple += cross2(pp, P[q == n ? 0 : q]);
                }
            }
            const unsigned long long b = __ballot(kept);
            if (lane == 0) wave_cnt[wave] = __popcll(b);
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int v = 0; v < SIMPLIFY_WAVES; ++v) {
                const int c = wave_cnt[v];
                if (v < wave) before += c;
                all += c;
            }
            __syncthreads();
            if (p < n) {
                w.rank[a + p] = kept ? carry + before + __popcll(b & ((1ull << lane) - 1ull)) : -1;
                w.loopof[a + p] = l;
            }
            carry += all;
        }
        exact = wave_sum64(exact);
        simple = wave_sum64(simple);
        if (lane == 0) {
            red[0][wave] = exact;
            red[1][wave] = simple;
        }
        __syncthreads();
        if (tid == 0) {
            exact = simple = 0;
#pragma unroll
            for (int v = 0; v < SIMPLIFY_WAVES; ++v) {
                exact += red[0][v];
                simple += red[1][v];
            }
            w.cnt[l] = carry >= 3 && simple != 0 ? carry : 0;
            w.lhole[l] = exact < 0 ? 1 : 0;
            w.rounds[l] = rounds;
        }
        __syncthreads();                                              // red and wave_cnt are free for the next loop
    }
}

// (1) split, form B: the loops of at most 64 corners, one wave per loop, four loops per workgroup at a time.  Lane p holds P_p,
//     the kept set is a 64-bit mask in every lane, i and j come from bit scans of it, the chain ends from two shuffles, and the
//     chain's (num, smallest k) from a segmented inclusive scan over the lanes of equal i in six shuffle steps, read from the
//     chain's last lane j - 1.  No LDS, no barrier.  Retired chains are worked out again every round: that costs nothing in a wave.
__global__ __launch_bounds__(VPU_SIMPLIFY_THREADS) void simplify_split_b_kernel(const int2* __restrict__ points, const int* __restrict__ offsets,
                                                                                const int* __restrict__ item_loops, int n_items, int V,
                                                                                int loop_max, int t, int32_t* __restrict__ work) {
    const SimplifyWork w = simplify_work(work, V, loop_max);
    const int lane = threadIdx.x & 63;
    const int L = clampi(item_loops[n_items], 0, loop_max);
    const unsigned long long below = (1ull << lane) - 1ull, above = lane == 63 ? 0ull : ~0ull << (lane + 1);
    for (int l = blockIdx.x * SIMPLIFY_WAVES + (threadIdx.x >> 6); l < L; l += gridDim.x * SIMPLIFY_WAVES) {
        int a, n;
        simplify_loop(offsets, l, V, a, n);
        if (n > VPU_SIMPLIFY_SHORT) continue;                         // (the same in every lane)
        const bool in = lane < n;
        const int2 pp = in ? points[a + lane] : make_int2(0, 0);
        unsigned long long kept = 1ull;
        int rounds = 0;
        long long tt = 0;                                             // S3: the first round is S4 with t = 0
        for (int r = 0; r <= n; ++r) {
            const bool live = in && !((kept >> lane) & 1ull);         // (lane 0 is kept, so a live lane has a kept one below)
            const int i = live ? 63 - __clzll((long long)(kept & below)) : -1;
            const int j = (kept & above) ? __ffsll((long long)(kept & above)) - 1 : n;
            const int ia = i < 0 ? 0 : i, jb = j >= n ? 0 : j;
            const int ax = __shfl(pp.x, ia, 64), ay = __shfl(pp.y, ia, 64), bx = __shfl(pp.x, jb, 64), by = __shfl(pp.y, jb, 64);
            long long num, den;
            simplify_distance(pp.x, pp.y, ax, ay, bx, by, num, den);
            long long bn = live ? num : -1;
            int bk = lane;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long on = __shfl_up(bn, o, 64);
                const int ok = __shfl_up(bk, o, 64), oi = __shfl_up(i, o, 64);
                if (live && lane >= o && oi == i && on >= bn) {       // (>=: the lower lanes win a tie)
                    bn = on;
                    bk = ok;
                }
            }
            const int last = clampi(j - 1, 0, 63);
            const long long cn = __shfl(bn, last, 64);
            const int ck = __shfl(bk, last, 64);
            const unsigned long long add = __ballot(live && ck == lane && 16 * cn > tt * den);       // S4; below 2^58
            if (!add) break;
            kept |= add;
            ++rounds;
            tt = (long long)t * t;
        }
        const bool mine = in && ((kept >> lane) & 1ull);
        const int nx = lane + 1 < n ? lane + 1 : 0;
        const int q = (kept & above) ? __ffsll((long long)(kept & above)) - 1 : 0;
        const int2 pn = make_int2(__shfl(pp.x, nx, 64), __shfl(pp.y, nx, 64)), pq = make_int2(__shfl(pp.x, q, 64), __shfl(pp.y, q, 64));
        const long long exact = wave_sum64(in ? cross2(pp, pn) : 0ll), simple = wave_sum64(mine ? cross2(pp, pq) : 0ll);
        const int count = n > 0 ? __popcll(kept) : 0;
        if (in) {
            w.rank[a + lane] = mine ? __popcll(kept & below) : -1;
            w.loopof[a + lane] = l;
        }
        if (lane == 0) {
            w.cnt[l] = count >= 3 && simple != 0 ? count : 0;
            w.lhole[l] = exact < 0 ? 1 : 0;
            w.rounds[l] = rounds;
        }
    }
}

// (2) offsets: ONE workgroup scans the loops' kept counts as in (2) of the trace: a surviving loop gets its index among the
//     survivors and its first point, writes its offset and its hole flag (below loop_cap); thread 0 the closing offset and the
//     totals {V', L', dropped, the most rounds of a loop}.
__global__ __launch_bounds__(1024) void simplify_offsets_kernel(const int* __restrict__ item_loops, int n_items, int V, int loop_max,
                                                                int32_t* __restrict__ work, int* __restrict__ out_offsets,
                                                                uint8_t* __restrict__ out_hole, int loop_cap, int* __restrict__ firsts) {
    __shared__ int wave_sum[16];
    __shared__ int most;
    const SimplifyWork w = simplify_work(work, V, loop_max);
    const int tid = threadIdx.x;
    const int L = clampi(item_loops[n_items], 0, loop_max);
    if (tid == 0) most = 0;
    __syncthreads();
    int loops = 0, pts = 0, mine = 0;                                 // (loops, pts: the same values in every thread)
    for (int off = 0; off < L; off += 4096) {
        const int i0 = off + 4 * tid;
        int c[4], alive[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = i0 + u < L ? clampi(w.cnt[i0 + u], 0, V) : 0;
            alive[u] = c[u] > 0 ? 1 : 0;
            if (i0 + u < L) mine = max(mine, w.rounds[i0 + u]);
        }
        int all_loops, all_pts;
        int at_loop = loops + block_scan(alive[0] + alive[1] + alive[2] + alive[3], wave_sum, all_loops);
        int at_pt = pts + block_scan(c[0] + c[1] + c[2] + c[3], wave_sum, all_pts);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u < L) {
                w.nidx[i0 + u] = at_loop;
                w.noff[i0 + u] = at_pt;
                if (alive[u] && (unsigned)at_loop < (unsigned)loop_cap) {
                    out_offsets[at_loop] = at_pt;
                    out_hole[at_loop] = (uint8_t)(w.lhole[i0 + u] != 0);
                }
            }
            at_loop += alive[u];
            at_pt += c[u];
        }
        loops += all_loops;
        pts += all_pts;
    }
    atomicMax(&most, mine);                                           // (LDS; after the barriers of block_scan or the one below)
    __syncthreads();
    if (tid == 0) {
        w.nidx[L] = loops;
        w.noff[L] = pts;
        if ((unsigned)loops < (unsigned)loop_cap) out_offsets[loops] = pts;
        int* tot = firsts + 2 * (n_items + 1);
        tot[0] = pts;
        tot[1] = loops;
        tot[2] = L - loops;
        tot[3] = most;
    }
}

// (3) place: every kept corner of a surviving loop stores its (x, y) with one 8-byte store at offset[loop'] + rank (below cap);
//     the first n + 1 threads write the items' first surviving loops and first points.  A corner counts only when the loop that
//     work names for it does hold it: then this call's split wrote its rank.
__global__ __launch_bounds__(256) void simplify_place_kernel(const int2* __restrict__ points, const int* __restrict__ offsets,
                                                             const int* __restrict__ item_loops, int n_items, int V, int loop_max,
                                                             const int32_t* __restrict__ work, int2* __restrict__ out_points, int cap,
                                                             int* __restrict__ firsts) {
    const SimplifyWork w = simplify_work(const_cast<int32_t*>(work), V, loop_max);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int L = clampi(item_loops[n_items], 0, loop_max);
    if (i <= n_items) {
        const int f = clampi(item_loops[i], 0, L);
        firsts[i] = w.nidx[f];
        firsts[n_items + 1 + i] = w.noff[f];
    }
    if (i >= V || L == 0) return;
    const int l = clampi(w.loopof[i], 0, L - 1);
    int a, n;
    simplify_loop(offsets, l, V, a, n);
    if (i < a || i >= a + n) return;
    const int r = w.rank[i], c = w.cnt[l];
    if (r < 0 || r >= c) return;
    const int at = w.noff[l] + r;
    if ((unsigned)at < (unsigned)cap) out_points[at] = points[i];
}

}  // namespace

extern "C" int vpu_outline_simplify_batched(const int32_t* points, const int32_t* offsets, const int32_t* item_loops, int32_t n, int32_t V,
                                            int32_t loop_max, int32_t t, int32_t short_form, int32_t* work, int64_t work_len,
                                            int32_t* out_points, int32_t cap, int32_t* out_offsets, int32_t loop_cap, uint8_t* out_hole,
                                            int32_t* firsts, void* stream) {
    vpu_clear_stale_error();
    if (!points || !offsets || !item_loops || !firsts || n < 1 || V < 0 || loop_max < 0 || cap < 0 || loop_cap < 0 ||
        (cap > 0 && !out_points) || (loop_cap > 0 && (!out_offsets || !out_hole))) {
        vpu_set_error("outline_simplify_batched: null points, offsets, item_loops, firsts, out_points, out_offsets or out_hole, n < 1, "
                      "or a negative V, loop_max or cap");
        return VPU_ERR_ARG;
    }
    if (t < 0 || t > 4096 || (short_form != 0 && short_form != 1)) {
        vpu_set_error("outline_simplify_batched: t outside 0 .. 4096 quarter pixels, or short_form not 0 (form A) or 1 (form B)");
        return VPU_ERR_ARG;
    }
    if (V > 0 && loop_max > 0 && (!work || work_len < VPU_SIMPLIFY_WORK_INTS(V, loop_max))) {
        vpu_set_error("outline_simplify_batched: null work or work_len below VPU_SIMPLIFY_WORK_INTS(V, loop_max)");
        return VPU_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(work) % 16 || reinterpret_cast<uintptr_t>(points) % 8 || reinterpret_cast<uintptr_t>(out_points) % 8 ||
        reinterpret_cast<uintptr_t>(offsets) % 8 || reinterpret_cast<uintptr_t>(out_offsets) % 8 ||
        reinterpret_cast<uintptr_t>(item_loops) % 4 || reinterpret_cast<uintptr_t>(firsts) % 4) {
        vpu_set_error("outline_simplify_batched: work not 16-byte, points, out_points, offsets or out_offsets not 8-byte, or item_loops "
                      "or firsts not 4-byte aligned");
        return VPU_ERR_ALIGN;
    }
    if (V == 0 || loop_max == 0) return 0;                            // no loop anywhere: nothing to launch
    const int2* pts = reinterpret_cast<const int2*>(points);
    const unsigned blocks_a = (unsigned)(loop_max < 2048 ? loop_max : 2048);
    simplify_split_a_kernel<<<blocks_a, VPU_SIMPLIFY_THREADS, 0, ST>>>(pts, offsets, item_loops, n, V, loop_max, t, short_form, work);
    if (short_form == 1) {
        const int64_t groups = ((int64_t)loop_max + SIMPLIFY_WAVES - 1) / SIMPLIFY_WAVES;
        simplify_split_b_kernel<<<(unsigned)(groups < 2048 ? groups : 2048), VPU_SIMPLIFY_THREADS, 0, ST>>>(pts, offsets, item_loops, n, V,
                                                                                                            loop_max, t, work);
    }
    simplify_offsets_kernel<<<1, 1024, 0, ST>>>(item_loops, n, V, loop_max, work, out_offsets, out_hole, loop_cap, firsts);
    const int64_t threads = V > n + 1 ? V : n + 1;
    simplify_place_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, ST>>>(pts, offsets, item_loops, n, V, loop_max, work,
                                                                            reinterpret_cast<int2*>(out_points), cap, firsts);
    return vpu_check_launch("vpu_outline_simplify_batched");
}
