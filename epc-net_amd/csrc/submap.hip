// Travel-length submaps from posed scans (include/epcnet_submaps.h: epcnet_submap_build; numpy restatement in tests/submap_ref.py): the
// step in front of the ground removal and the down-sampler.  The definition is float64 with every operation rounded once (contract off),
// one rounding to float32 at the end and integer counts, so the result is the same bits on every run and equal to numpy's.
//
// offsets, poses and along are device data: every grid is sized from num_scans, max_submaps and out_rows alone.
//   scan_clear_words       clears the workspace's head (scan_common.h: a launch, not a memset)
//   submap_check_kernel    one thread per scan: the offsets' rule, along finite and non-decreasing; an integer OR into one word that the
//                          launch before it cleared
//   submap_seg_kernel      one thread per slot (and one for slot max_submaps, which only says whether the trajectory goes on): c, s, e,
//                          the three lower bounds in `along`, rows_k, sub_pose, sub_info
//   submap_layout_kernel   ONE workgroup: the exclusive integer scan of rows_k in chunks of its width with a running carry, the fit rule,
//                          sub_offsets, status, num_out
//   submap_gather_kernel   the hot path.  Flat tiles of SM_TILE OUTPUT rows over [0, out_rows): a tile finds its slot in sub_offsets and
//                          its scan in offsets by binary search ONCE (thread 0), then walks on from there and lists the (submap, scan)
//                          pairs it touches in LDS, SM_PAIRS at a time; twelve threads per pair build M | u in LDS (27 + 9 products per
//                          PAIR, not per row).  The rows of a batch come in as whole dwords across the wave (dword d of the tile from
//                          dword d of the source: a submap's rows are contiguous in the source) into an LDS image, every thread
//                          transforms rows of the image in place (stride 3 dwords: no bank conflict), and the image leaves as whole
//                          dwords again.  No global atomics, no float atomics anywhere.
#include "scan_common.h"
#include "../../include/epcnet_submaps.h"

#define SM_THREADS 256
#define SM_TILE 1024           // output rows per gather tile (tests/test_gpu_submap.py names it T): a 12 KB LDS image
#define SM_PAIRS 32            // (submap, scan) pairs listed at a time; a tile with more of them takes several batches
#define SM_SCAN_THREADS 1024   // the layout kernel's one workgroup
#define SM_HEAD 4              // workspace words in front: [0] the whole-call failure

// the workspace: head (4 int32) | P (max_submaps + 1 int64) | seg (max_submaps + 1 slots of lo hi ref rows, int32)
struct sm_ws {
    int32_t* head;
    long long* P;
    int32_t* seg;
};
__host__ __device__ __forceinline__ sm_ws sm_carve(void* workspace, int max_submaps) {
    sm_ws w;
    w.head = reinterpret_cast<int32_t*>(workspace);
    w.P = reinterpret_cast<long long*>(w.head + SM_HEAD);
    w.seg = reinterpret_cast<int32_t*>(w.P + ((size_t)max_submaps + 1));
    return w;
}
static size_t sm_ws_bytes(int max_submaps) {
    return SM_HEAD * sizeof(int32_t) + ((size_t)max_submaps + 1) * (sizeof(long long) + 4 * sizeof(int32_t));
}

struct sm_params {
    double h, spacing, min2, max2, z_min, z_max;
};

// ---- launch 1: the whole-call failures ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_THREADS) void submap_check_kernel(const int32_t* __restrict__ offsets, const double* __restrict__ along,
                                                                  long long num_rows, int num_scans, sm_ws ws) {
    const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    int bad = ((i == 0 && num_scans == 0) || offsets_rule_bad(offsets, num_scans, num_rows, i)) ? 1 : 0;      // no scan: a failed call
    if (i < num_scans) {
        const double a = along[i];
        bad |= __builtin_isfinite(a) ? 0 : 1;
        if (i + 1 < num_scans) bad |= a <= along[i + 1] ? 0 : 1;          // (a NaN behind it is bad in its own thread)
    }
    if (bad) atomicOr(&ws.head[0], 1);
}

// the first i in [0, n) with along[i] >= v (n when there is none); along is non-decreasing here
__device__ __forceinline__ int sm_lower_bound(const double* __restrict__ along, int n, double v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (along[mid] >= v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// ---- launch 2: the slots --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_THREADS) void submap_seg_kernel(const int32_t* __restrict__ offsets, const double* __restrict__ poses,
                                                                const double* __restrict__ along, int num_scans, int max_submaps,
                                                                sm_params pr, sm_ws ws, double* __restrict__ sub_pose,
                                                                int32_t* __restrict__ sub_info) {
    const int k = blockIdx.x * SM_THREADS + threadIdx.x;
    if (k > max_submaps) return;
    int lo = -1, hi = -1, ref = -1, rows = 0;
    if (ws.head[0] == 0) {                             // (a valid call has num_scans >= 1)
#pragma clang fp contract(off)
        const double c = (along[0] + pr.h) + (double)k * pr.spacing;
        const double s = c - pr.h, e = c + pr.h;
        if (e <= along[num_scans - 1]) {
            lo = sm_lower_bound(along, num_scans, s);
            hi = sm_lower_bound(along, num_scans, e);
            ref = sm_lower_bound(along, num_scans, c);
            rows = offsets[hi] - offsets[lo];
            if (rows > EPC_SUBMAP_MAX_ROWS) rows = -1;                     // a submap, of no row: NO_ROOM (the layout kernel's word)
        }
    }
    int32_t* g = ws.seg + (size_t)k * 4;
    g[0] = lo, g[1] = hi, g[2] = ref, g[3] = rows;
    if (k == max_submaps) return;                      // the slot behind the last one has no outputs
    const double nan = epc_nan_f64();
    for (int c = 0; c < 12; ++c) sub_pose[(size_t)k * 12 + c] = ref >= 0 ? poses[(size_t)ref * 12 + c] : nan;
    if (sub_info) {
        int32_t* o = sub_info + (size_t)k * 4;
        o[0] = lo, o[1] = hi, o[2] = ref, o[3] = rows > 0 ? rows : 0;
    }
}

// ---- launch 3: the layout -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_SCAN_THREADS) void submap_layout_kernel(int max_submaps, long long out_rows, sm_ws ws,
                                                                        int32_t* __restrict__ sub_offsets, int32_t* __restrict__ num_out,
                                                                        int32_t* __restrict__ status) {
    __shared__ long long part[SM_SCAN_THREADS / 64];
    __shared__ long long fit_end;                      // P[k_fit]
    __shared__ int count;                              // the submaps among the slots
    const int tid = threadIdx.x;
    if (tid == 0) fit_end = 0, count = 0;
    // pass 1: P, the end of the submaps that fit, the number of submaps
    long long carry = 0, my_fit = 0;
    int my_count = 0;
    for (int base = 0; base < max_submaps; base += SM_SCAN_THREADS) {
        const int k = base + tid;
        const int rows = k < max_submaps ? ws.seg[(size_t)k * 4 + 3] : 0;
        const bool is_submap = k < max_submaps && ws.seg[(size_t)k * 4] >= 0;
        const long long v = rows > 0 ? rows : 0;
        long long total;
        const long long excl = carry + block_scan<SM_SCAN_THREADS / 64>(v, part, total), incl = excl + v;
        if (k < max_submaps) ws.P[k] = excl;
        if (is_submap) {
            ++my_count;
            if (incl <= out_rows && incl > my_fit) my_fit = incl;          // P[k + 1] of a submap that fits (P is monotone: the largest)
        }
        carry += total;
    }
    if (tid == 0) ws.P[max_submaps] = carry;
    if (my_count) atomicAdd(&count, my_count);
    if (my_fit) atomicMax(reinterpret_cast<unsigned long long*>(&fit_end), (unsigned long long)my_fit);
    __syncthreads();
    // pass 2: the words.  A submap fits iff P[k + 1] <= out_rows, which for a monotone P is P[k + 1] <= P[k_fit]
    const long long end = fit_end;
    for (int k = tid; k <= max_submaps; k += SM_SCAN_THREADS) {
        const long long p = ws.P[k];
        sub_offsets[k] = (int32_t)(p < end ? p : end);
        if (k < max_submaps) {
            const int rows = ws.seg[(size_t)k * 4 + 3];
            const bool is_submap = ws.seg[(size_t)k * 4] >= 0;
            const long long next = p + (rows > 0 ? rows : 0);
            status[k] = !is_submap ? EPC_STATUS_NO_SUBMAP : (rows < 0 || next > out_rows) ? EPC_STATUS_NO_ROOM : 0;
        }
    }
    if (tid == 0) {
        num_out[0] = count;
        num_out[1] = ws.seg[(size_t)max_submaps * 4] >= 0 ? 1 : 0;
    }
}

// ---- launch 4: the rows ---------------------------------------------------------------------------------------------------------------
// q_a and the keep rule of one row; returns the three output words.  (Not st_row of stamps.hip: another layout, another association)
__device__ __forceinline__ void sm_row(const double* __restrict__ m, const sm_params& pr, float xf, float yf, float zf, float* ox,
                                       float* oy, float* oz) {
#pragma clang fp contract(off)
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double rr = (x * x + y * y) + z * z;
    const double q0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[9];
    const double q1 = ((m[3] * x + m[4] * y) + m[5] * z) + m[10];
    const double q2 = ((m[6] * x + m[7] * y) + m[8] * z) + m[11];
    const bool keep = rr >= pr.min2 && (q0 * q0 + q1 * q1) <= pr.max2 && pr.z_min <= q2 && q2 <= pr.z_max;
    const float nan = epc_nan_f32();
    *ox = keep ? (float)q0 : nan;
    *oy = keep ? (float)q1 : nan;
    *oz = keep ? (float)q2 : nan;
}

// entry e of a pair's M | u: M[a][b] at 3a + b, u[a] at 9 + a.  (Not st_pose_at of stamps.hip: another published definition)
__device__ __forceinline__ double sm_pair_entry(const double* __restrict__ Ri, const double* __restrict__ Rr, int e) {
#pragma clang fp contract(off)
    if (e < 9) {
        const int a = e / 3, b = e - 3 * a;
        return (Rr[a] * Ri[b] + Rr[4 + a] * Ri[4 + b]) + Rr[8 + a] * Ri[8 + b];
    }
    const int a = e - 9;
    const double d0 = Ri[3] - Rr[3], d1 = Ri[7] - Rr[7], d2 = Ri[11] - Rr[11];
    return (Rr[a] * d0 + Rr[4 + a] * d1) + Rr[8 + a] * d2;
}

__global__ __launch_bounds__(SM_THREADS) void submap_gather_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                   const double* __restrict__ poses, int max_submaps, sm_params pr,
                                                                   sm_ws ws, const int32_t* __restrict__ sub_offsets,
                                                                   float* __restrict__ out) {
    __shared__ float img[SM_TILE * 3];
    __shared__ double mu[SM_PAIRS][12];
    __shared__ int p_out[SM_PAIRS + 1];                // the pair's first row, tile-local; [np]: the batch's end
    __shared__ int p_src[SM_PAIRS];                    // the source row of that row
    __shared__ int p_scan[SM_PAIRS], p_ref[SM_PAIRS];
    __shared__ int np_s;
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * SM_TILE;
    const long long total = sub_offsets[max_submaps];
    if (t0 >= total) return;                           // (uniform)
    const int rows_here = (int)(t0 + SM_TILE < total ? SM_TILE : total - t0);

    // thread 0's walk: the slot k and the scan i of tile-local row `at`.  (Not shared with the walk of stamps.hip: this one steps over slots too)
    int k = 0, i = 0;
    if (tid == 0) {
        k = first_scan_behind(sub_offsets, 0, max_submaps, t0);          // the first slot whose end lies behind row t0 (it exists: t0 < total)
        const int32_t* g = ws.seg + (size_t)k * 4;
        const int src = offsets[g[0]] + (int)(t0 - sub_offsets[k]);
        i = first_scan_behind(offsets, g[0], g[1], src);                 // the first scan of the slot whose end lies behind row src
    }
    for (int at = 0; at < rows_here;) {
        if (tid == 0) {
            int np = 0, r = at;
            while (np < SM_PAIRS && r < rows_here) {
                const int32_t* g = ws.seg + (size_t)k * 4;
                const int first = offsets[g[0]], k_begin = sub_offsets[k];
                const long long row = t0 + r;
                const long long scan_end = (long long)k_begin + (offsets[i + 1] - first);      // in output rows
                const int e = (int)((scan_end < t0 + rows_here ? scan_end : t0 + rows_here) - t0);
                p_out[np] = r, p_src[np] = first + (int)(row - k_begin), p_scan[np] = i, p_ref[np] = g[2];
                ++np;
                r = e;
                if (r >= rows_here) break;
                // the next scan with a row, in this slot or in the next slot that has rows (there is one: r < rows_here <= total - t0)
                ++i;
                for (;;) {
                    const int32_t* gk = ws.seg + (size_t)k * 4;
                    while (i < gk[1] && offsets[i + 1] == offsets[i]) ++i;
                    if (i < gk[1] && t0 + r < (long long)sub_offsets[k + 1]) break;
                    do ++k; while (sub_offsets[k + 1] == sub_offsets[k]);
                    i = ws.seg[(size_t)k * 4];
                }
            }
            p_out[np] = r;
            np_s = np;
        }
        __syncthreads();
        const int np = np_s, b0 = at, b1 = p_out[np];
        for (int e = tid; e < 12 * np; e += SM_THREADS) {
            const int p = e / 12;
            mu[p][e - 12 * p] = sm_pair_entry(poses + (size_t)p_scan[p] * 12, poses + (size_t)p_ref[p] * 12, e - 12 * p);
        }
        // the batch's dwords in: dword d of the tile from the pair that holds its row
        for (int d = 3 * b0 + tid; d < 3 * b1; d += SM_THREADS) {
            const int row = d / 3;
            const int lo = pair_of_row(p_out, np, row);
            img[d] = points[(size_t)p_src[lo] * 3 + (size_t)(d - 3 * p_out[lo])];
        }
        __syncthreads();
        for (int row = b0 + tid; row < b1; row += SM_THREADS) {
            const int lo = pair_of_row(p_out, np, row);
            float ox, oy, oz;
            sm_row(mu[lo], pr, img[3 * row], img[3 * row + 1], img[3 * row + 2], &ox, &oy, &oz);
            img[3 * row] = ox, img[3 * row + 1] = oy, img[3 * row + 2] = oz;
        }
        __syncthreads();
        float* o = out + (size_t)t0 * 3;
        for (int d = 3 * b0 + tid; d < 3 * b1; d += SM_THREADS) o[d] = img[d];
        at = b1;
        __syncthreads();                               // (the lists and the image are free again)
    }
}

static bool sm_supported(int num_scans, int max_submaps, long long num_rows, long long out_rows) {
    return num_scans >= 0 && num_scans <= (1 << 24) && max_submaps >= 1 && max_submaps <= 65535 && num_rows >= 0 && out_rows >= 0 &&
           out_rows < 2147483648ll;
}

extern "C" size_t epcnet_submap_workspace_bytes(int num_scans, int max_submaps, long long num_rows, long long out_rows) {
    if (!sm_supported(num_scans, max_submaps, num_rows, out_rows)) return 0;
    return sm_ws_bytes(max_submaps);
}

extern "C" int epcnet_submap_build(const float* points, const int32_t* offsets, long long num_rows, int num_scans, const double* poses,
                                   const double* along, const double* params, int max_submaps, long long out_rows, float* points_out,
                                   int32_t* sub_offsets, int32_t* num_out, double* sub_pose, int32_t* sub_info, int32_t* status,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && poses && along && params && points_out && sub_offsets && num_out && sub_pose && status && workspace,
                  "null pointer");
    EPC_CHECK_ARG(num_rows >= 0, "num_rows must not be negative");
    EPC_CHECK_ARG(num_scans >= 0 && num_scans <= (1 << 24), "need 0 <= num_scans <= 2^24");
    EPC_CHECK_ARG(max_submaps >= 1 && max_submaps <= 65535, "need 1 <= max_submaps <= 65535");
    EPC_CHECK_ARG(out_rows >= 0 && out_rows < 2147483648ll, "need 0 <= out_rows < 2^31");
    const double length = params[0], spacing = params[1], min_range = params[2], max_range = params[3], z_min = params[4],
                 z_max = params[5];
    EPC_CHECK_ARG(__builtin_isfinite(length) && length > 0.0, "length must be finite and > 0");
    EPC_CHECK_ARG(__builtin_isfinite(spacing) && spacing > 0.0, "spacing must be finite and > 0");
    EPC_CHECK_ARG(min_range >= 0.0, "min_range must be >= 0");
    EPC_CHECK_ARG(__builtin_isfinite(max_range) && max_range > 0.0, "max_range must be finite and > 0");
    EPC_CHECK_ARG(z_min == z_min && z_max == z_max, "z_min and z_max must not be NaN (-Inf, +Inf: no limit)");
    EPC_CHECK_ARG(params[6] == 0.0 && params[7] == 0.0, "the two reserved parameters must be 0");
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_submap_workspace_bytes(num_scans, max_submaps, num_rows, out_rows));
    sm_params pr;
    {
#pragma clang fp contract(off)
        pr.h = length * 0.5;
        pr.spacing = spacing;
        pr.min2 = min_range * min_range;
        pr.max2 = max_range * max_range;
        pr.z_min = z_min;
        pr.z_max = z_max;
    }
    hipStream_t st = (hipStream_t)stream;
    const sm_ws ws = sm_carve(workspace, max_submaps);
    if (int rc = scan_clear_words_launch(ws.head, SM_HEAD, st, __func__)) return rc;
    const int check_blocks = num_scans > 0 ? (num_scans + SM_THREADS - 1) / SM_THREADS : 1;
    hipLaunchKernelGGL(submap_check_kernel, dim3(check_blocks), dim3(SM_THREADS), 0, st, offsets, along, num_rows, num_scans, ws);
    EPC_CHECK_LAUNCH();
    hipLaunchKernelGGL(submap_seg_kernel, dim3((max_submaps + 1 + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0, st, offsets, poses,
                       along, num_scans, max_submaps, pr, ws, sub_pose, sub_info);
    EPC_CHECK_LAUNCH();
    hipLaunchKernelGGL(submap_layout_kernel, dim3(1), dim3(SM_SCAN_THREADS), 0, st, max_submaps, out_rows, ws, sub_offsets, num_out, status);
    EPC_CHECK_LAUNCH();
    const int tiles = (int)((out_rows + SM_TILE - 1) / SM_TILE);
    if (tiles > 0) {
        hipLaunchKernelGGL(submap_gather_kernel, dim3(tiles), dim3(SM_THREADS), 0, st, points, offsets, poses, max_submaps, pr, ws,
                           sub_offsets, points_out);
        EPC_CHECK_LAUNCH();
    }
    return EPC_OK;
}
