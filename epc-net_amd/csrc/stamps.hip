// Timestamped scans (include/epcnet_stamps.h: epcnet_pose_interp, epcnet_scan_deskew; numpy restatement in tests/stamps_ref.py): the
// step in front of the submap build.  The definition is integer times, float64 with every operation rounded once (contract off), one
// correctly rounded division per pose and one rounding to float32 at the end, so the result is the same bits on every run and equal to
// numpy's.
//
// offsets, the times and the poses are device data: every grid is sized from num_scans (num_queries), num_poses and num_rows alone.
//   scan_clear_words      clears the workspace's head (scan_common.h: a launch, not a memset)
//   stamps_check_kernel   one thread per scan and per pose: the offsets' rule, pose_time strictly increasing; an integer OR into one word
//                         that the launch before it cleared
//   stamps_scan_kernel    one thread per scan (query): the bracket index j_i by binary search, the pose at the scan's time, the status
//                         word, and j_i (-1: the scan's pose is invalid) for the row kernel.  epcnet_pose_interp shares it
//   stamps_row_kernel     the hot path.  Flat tiles of ST_TILE rows over [0, num_rows): rows and point_dt come in as whole dwords across
//                         the wave into an LDS image; thread 0 finds the tile's first scan in offsets by ONE binary search, walks on and
//                         lists the (scan, row range) pairs in LDS, ST_PAIRS at a time, with each pair's j_i, time and pose; every thread
//                         finds its row's bracket by galloping outward from its scan's j_i (point_dt is small against a pose interval:
//                         1 - 3 steps; the result is the definition's unique index whatever the order), blends, builds Rp and transforms
//                         its row of the image in place (stride 3 dwords: no bank conflict); the image leaves as whole dwords.  The only
//                         atomic is the integer OR of EPC_STATUS_PART_POSE.
#include "scan_common.h"
#include "../../include/epcnet_stamps.h"

#define ST_THREADS 256
#define ST_TILE 1024           // rows per tile (tests/test_gpu_stamps.py names it T): a 12 KB image and 4 KB of point_dt in LDS
#define ST_PAIRS 32            // (scan, row range) pairs listed at a time; a tile with more of them takes several batches
#define ST_HEAD 4              // workspace words in front: [0] the whole-call failure

// the workspace: head (4 int32) | j (num_scans int32), rounded up to 16 bytes (the head is 16 bytes itself)
struct st_ws { int32_t *head, *scan_j; size_t bytes; };
static st_ws st_layout(void* base, int num_scans) {
    epc_carver c(base);
    return {c.take<int32_t>(ST_HEAD), c.take<int32_t>(num_scans, 16), c.bytes()};
}

// ---- the definition -------------------------------------------------------------------------------------------------------------------
// floor(num * 2^32 / den) for 0 <= num <= den < 2^31, den > 0: a float64 estimate (off by one at most) put right in integers
__device__ __forceinline__ unsigned long long st_fraction(unsigned long long num, unsigned long long den) {
    const unsigned long long x = num << 32;                                // (31 significant bits: exact as a double)
    unsigned long long q = (unsigned long long)((double)x / (double)den);
    long long r = (long long)(x - q * den);
    while (r < 0) --q, r += (long long)den;
    while (r >= (long long)den) ++q, r -= (long long)den;
    return q;
}

// the pose at time tau in bracket j as [R | t] in m[12]; false, and twelve NaN words, when it is invalid.  (Not sm_pair_entry of
// submap.hip: another published definition)
__device__ __forceinline__ bool st_pose_at(const long long* __restrict__ pose_time, const double* __restrict__ pose, int j, long long tau,
                                           long long max_gap, double* m) {
#pragma clang fp contract(off)
    bool ok = false;
    if (j >= 0) {
        const long long ta = pose_time[j], tb = pose_time[j + 1];
        const long long num = (long long)((unsigned long long)tau - (unsigned long long)ta);
        const long long den = (long long)((unsigned long long)tb - (unsigned long long)ta);
        if (num >= 0 && num <= den && den <= max_gap && den > 0) {
            const double f = (double)st_fraction((unsigned long long)num, (unsigned long long)den) * 0x1p-32;
            const double g = 1.0 - f;
            const double* __restrict__ p0 = pose + (size_t)j * 7;
            const double* __restrict__ p1 = p0 + 7;
            const double t0 = p0[0] + f * (p1[0] - p0[0]);
            const double t1 = p0[1] + f * (p1[1] - p0[1]);
            const double t2 = p0[2] + f * (p1[2] - p0[2]);
            const double w0 = p0[3], x0 = p0[4], y0 = p0[5], z0 = p0[6];
            double w1 = p1[3], x1 = p1[4], y1 = p1[5], z1 = p1[6];
            const double d = ((w0 * w1 + x0 * x1) + y0 * y1) + z0 * z1;
            if (d < 0.0) w1 = -w1, x1 = -x1, y1 = -y1, z1 = -z1;
            const double w = g * w0 + f * w1;
            const double x = g * x0 + f * x1;
            const double y = g * y0 + f * y1;
            const double z = g * z0 + f * z1;
            const double n = ((w * w + x * x) + y * y) + z * z;
            const double s = 2.0 / n;
            m[0] = 1.0 - s * (y * y + z * z);
            m[1] = s * (x * y - w * z);
            m[2] = s * (x * z + w * y);
            m[3] = t0;
            m[4] = s * (x * y + w * z);
            m[5] = 1.0 - s * (x * x + z * z);
            m[6] = s * (y * z - w * x);
            m[7] = t1;
            m[8] = s * (x * z - w * y);
            m[9] = s * (y * z + w * x);
            m[10] = 1.0 - s * (x * x + y * y);
            m[11] = t2;
            ok = __builtin_isfinite(n) && n > 0.0 && __builtin_isfinite(t0) && __builtin_isfinite(t1) && __builtin_isfinite(t2);
        }
    }
    if (!ok) {
        const double nan = epc_nan_f64();
#pragma unroll
        for (int c = 0; c < 12; ++c) m[c] = nan;
    }
    return ok;
}

// q_a of one row: the pose (rp) at the row's own time, the pose (rs) at its scan's.  (Not sm_row of submap.hip: another layout, another
// association of the sums)
__device__ __forceinline__ void st_row(const double* rp, const double* __restrict__ rs, float xf, float yf, float zf, float* ox, float* oy,
                                       float* oz) {
#pragma clang fp contract(off)
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double w0 = ((rp[0] * x + rp[1] * y) + rp[2] * z) + (rp[3] - rs[3]);
    const double w1 = ((rp[4] * x + rp[5] * y) + rp[6] * z) + (rp[7] - rs[7]);
    const double w2 = ((rp[8] * x + rp[9] * y) + rp[10] * z) + (rp[11] - rs[11]);
    *ox = (float)((rs[0] * w0 + rs[4] * w1) + rs[8] * w2);
    *oy = (float)((rs[1] * w0 + rs[5] * w1) + rs[9] * w2);
    *oz = (float)((rs[2] * w0 + rs[6] * w1) + rs[10] * w2);
}

// ---- launch 1: the whole-call failures ------------------------------------------------------------------------------------------------
// offsets may be NULL (epcnet_pose_interp: the order of pose_time alone)
__global__ __launch_bounds__(ST_THREADS) void stamps_check_kernel(const int32_t* __restrict__ offsets, long long num_rows, int num_scans,
                                                                  const long long* __restrict__ pose_time, int num_poses, int32_t* flag) {
    const long long i = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
    int bad = (offsets && offsets_rule_bad(offsets, num_scans, num_rows, i)) ? 1 : 0;
    if (i + 1 < num_poses) bad |= pose_time[i] < pose_time[i + 1] ? 0 : 1;
    if (bad) atomicOr(flag, EPC_STATUS_NO_POSE);
}

// ---- launch 2: the scans (queries) ------------------------------------------------------------------------------------------------------
// queries [first, first + count).  `flag` is the workspace's word, or status itself (epcnet_pose_interp: status[0] carries the verdict
// until the query 0 is written, in a launch of its own behind all the others), so neither pointer is __restrict__
__global__ __launch_bounds__(ST_THREADS) void stamps_scan_kernel(const long long* __restrict__ query_time,
                                                                 const long long* __restrict__ pose_time, const double* __restrict__ pose,
                                                                 int num_poses, long long max_gap, const int32_t* flag, int first,
                                                                 int count, double* __restrict__ pose_out, int32_t* status,
                                                                 int32_t* __restrict__ j_out) {
    const long long at = (long long)blockIdx.x * ST_THREADS + threadIdx.x;
    if (at >= count) return;
    const int i = first + (int)at;
    int j = -1;
    if (flag[0] == 0) {
        const long long tau = query_time[i];
        int lo = 0, hi = num_poses;                    // the number of pose times at or before tau
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pose_time[mid] <= tau)
                lo = mid + 1;
            else
                hi = mid;
        }
        j = lo - 1 < num_poses - 2 ? lo - 1 : num_poses - 2;
        double m[12];
        const bool ok = st_pose_at(pose_time, pose, j, tau, max_gap, m);
#pragma unroll
        for (int c = 0; c < 12; ++c) pose_out[(size_t)i * 12 + c] = m[c];
        if (!ok) j = -1;
    } else {
        const double nan = epc_nan_f64();
        for (int c = 0; c < 12; ++c) pose_out[(size_t)i * 12 + c] = nan;
    }
    status[i] = j >= 0 ? 0 : EPC_STATUS_NO_POSE;
    if (j_out) j_out[i] = j;
}

// ---- launch 3: the rows -----------------------------------------------------------------------------------------------------------------
// the definition's j for tau, found from a start index js in [0, num_poses - 2] by galloping outward and bisecting: -1 .. num_poses - 2
__device__ __forceinline__ int st_bracket(const long long* __restrict__ pose_time, int num_poses, int js, long long tau) {
    int lo, hi;                                        // pose_time[lo] <= tau (or lo == -1) and pose_time[hi] > tau (or hi == num_poses - 1)
    if (pose_time[js] <= tau) {
        lo = js, hi = js + 1;
        for (int step = 1; hi < num_poses - 1 && pose_time[hi] <= tau; step <<= 1) {
            lo = hi;
            hi = hi + 2 * step < num_poses - 1 ? hi + 2 * step : num_poses - 1;
        }
    } else {
        hi = js, lo = js - 1;
        for (int step = 1; lo >= 0 && pose_time[lo] > tau; step <<= 1) {
            hi = lo;
            lo = lo - 2 * step > -1 ? lo - 2 * step : -1;
        }
    }
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pose_time[mid] <= tau)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ST_THREADS) void stamps_row_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                int num_scans, const int32_t* __restrict__ point_dt,
                                                                const long long* __restrict__ scan_time,
                                                                const long long* __restrict__ pose_time, const double* __restrict__ pose,
                                                                int num_poses, long long max_gap, const double* __restrict__ scan_pose,
                                                                const int32_t* __restrict__ head, const int32_t* __restrict__ scan_j,
                                                                int32_t* status, float* __restrict__ out) {
    __shared__ float img[ST_TILE * 3];
    __shared__ int32_t dts[ST_TILE];
    __shared__ double sp[ST_PAIRS][12];                // the pair's scan pose
    __shared__ long long p_time[ST_PAIRS];
    __shared__ int p_out[ST_PAIRS + 1];                // the pair's first row, tile-local; [np]: the batch's end
    __shared__ int p_scan[ST_PAIRS], p_j[ST_PAIRS];
    __shared__ int np_s;
    const int tid = threadIdx.x;
    if (head[0] != 0 || num_scans == 0) return;        // (uniform) the whole call failed: no row is written
    const long long t0 = (long long)blockIdx.x * ST_TILE;
    const long long first = offsets[0], last = offsets[num_scans];
    const long long r_lo = t0 > first ? t0 : first, r_hi = t0 + ST_TILE < last ? t0 + ST_TILE : last;
    if (r_lo >= r_hi) return;                          // (uniform) no row of a scan in this tile
    const int a = (int)(r_lo - t0), b = (int)(r_hi - t0);

    const float* src = points + (size_t)t0 * 3;
    for (int d = 3 * a + tid; d < 3 * b; d += ST_THREADS) img[d] = src[d];
    for (int r = a + tid; r < b; r += ST_THREADS) dts[r] = point_dt[(size_t)t0 + r];

    int i = 0;                                         // thread 0's walk: the scan of tile-local row `at` (submap.hip's walk steps over slots too)
    if (tid == 0) {
        i = first_scan_behind(offsets, 0, num_scans - 1, r_lo);          // the first scan whose end lies behind row r_lo (it exists: r_lo < last)
    }
    for (int at = a; at < b;) {
        if (tid == 0) {
            int np = 0, r = at;
            while (np < ST_PAIRS && r < b) {
                const long long scan_end = (long long)offsets[i + 1] - t0;
                p_out[np] = r, p_scan[np] = i;
                ++np;
                r = scan_end < b ? (int)scan_end : b;
                if (r >= b) break;
                ++i;                                   // the next scan with a row (there is one: t0 + r < last)
                while (offsets[i + 1] == offsets[i]) ++i;
            }
            p_out[np] = r;
            np_s = np;
        }
        __syncthreads();                               // (also: the image and dts are in)
        const int np = np_s, b1 = p_out[np];
        for (int e = tid; e < 12 * np; e += ST_THREADS) {
            const int p = e / 12;
            sp[p][e - 12 * p] = scan_pose[(size_t)p_scan[p] * 12 + (e - 12 * p)];
        }
        for (int p = tid; p < np; p += ST_THREADS) p_j[p] = scan_j[p_scan[p]], p_time[p] = scan_time[p_scan[p]];
        __syncthreads();
        for (int row = at + tid; row < b1; row += ST_THREADS) {
            const int lo = pair_of_row(p_out, np, row);
            const float nanf = epc_nan_f32();
            float ox = nanf, oy = nanf, oz = nanf;
            const int js = p_j[lo];
            if (js >= 0) {                             // the scan's pose is valid
                const long long tau = (long long)((unsigned long long)p_time[lo] + (unsigned long long)(long long)dts[row]);
                double m[12];
                const bool ok = st_pose_at(pose_time, pose, st_bracket(pose_time, num_poses, js, tau), tau, max_gap, m);
                if (!ok) atomicOr(&status[p_scan[lo]], EPC_STATUS_PART_POSE);
                const float x = img[3 * row], y = img[3 * row + 1], z = img[3 * row + 2];
                const bool finite = epc_finite3(x, y, z);      // (named: inside the condition hipcc takes 126 VGPRs for this kernel, not 68)
                if (ok && finite) st_row(m, sp[lo], x, y, z, &ox, &oy, &oz);
            }
            img[3 * row] = ox, img[3 * row + 1] = oy, img[3 * row + 2] = oz;
        }
        at = b1;
        __syncthreads();                               // (the lists are free again; behind the last batch: the image is whole)
    }
    float* o = out + (size_t)t0 * 3;
    for (int d = 3 * a + tid; d < 3 * b; d += ST_THREADS) o[d] = img[d];
}

// ---- the entries ------------------------------------------------------------------------------------------------------------------------
static bool st_supported(int num_scans, int num_poses, long long num_rows) {
    return num_scans >= 0 && num_scans <= (1 << 24) && num_poses >= 2 && num_poses <= (1 << 24) && num_rows >= 0 && num_rows < 2147483648ll;
}

extern "C" size_t epcnet_deskew_workspace_bytes(int num_scans, int num_poses, long long num_rows) {
    if (!st_supported(num_scans, num_poses, num_rows)) return 0;
    return st_layout(nullptr, num_scans).bytes;
}

static int st_blocks(long long n) { return (int)((n + ST_THREADS - 1) / ST_THREADS); }

extern "C" int epcnet_pose_interp(const long long* pose_time, const double* pose, int num_poses, const long long* query_time,
                                  int num_queries, long long max_gap_ns, double* pose_out, int32_t* status, void* stream) {
    EPC_CHECK_ARG(pose_time && pose && query_time && pose_out && status, "null pointer");
    EPC_CHECK_ARG(num_poses >= 2 && num_poses <= (1 << 24), "need 2 <= num_poses <= 2^24");
    EPC_CHECK_ARG(num_queries >= 0 && num_queries <= (1 << 24), "need 0 <= num_queries <= 2^24");
    EPC_CHECK_ARG(max_gap_ns >= 1 && max_gap_ns < 2147483648ll, "need 1 <= max_gap_ns < 2^31");
    if (num_queries == 0) return EPC_OK;
    hipStream_t st = (hipStream_t)stream;
    // status[0] is the check's word until query 0 is written, behind all the others
    if (int rc = scan_clear_words_launch(status, 1, st, __func__)) return rc;
    hipLaunchKernelGGL(stamps_check_kernel, dim3(st_blocks(num_poses)), dim3(ST_THREADS), 0, st, (const int32_t*)nullptr, 0ll, 0, pose_time,
                       num_poses, status);
    EPC_CHECK_LAUNCH();
    if (num_queries > 1) {
        hipLaunchKernelGGL(stamps_scan_kernel, dim3(st_blocks(num_queries - 1)), dim3(ST_THREADS), 0, st, query_time, pose_time, pose,
                           num_poses, max_gap_ns, (const int32_t*)status, 1, num_queries - 1, pose_out, status, (int32_t*)nullptr);
        EPC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(stamps_scan_kernel, dim3(1), dim3(ST_THREADS), 0, st, query_time, pose_time, pose, num_poses, max_gap_ns,
                       (const int32_t*)status, 0, 1, pose_out, status, (int32_t*)nullptr);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

extern "C" int epcnet_scan_deskew(const float* points, const int32_t* offsets, long long num_rows, int num_scans, const int32_t* point_dt,
                                  const long long* scan_time, const long long* pose_time, const double* pose, int num_poses,
                                  long long max_gap_ns, float* points_out, double* scan_pose, int32_t* status, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && scan_time && pose_time && pose && scan_pose && status && workspace, "null pointer");
    EPC_CHECK_ARG(!point_dt || points_out, "points_out may be NULL only when point_dt is");
    EPC_CHECK_ARG(!point_dt || points_out != points, "points_out must not be points");
    EPC_CHECK_ARG(num_rows >= 0 && num_rows < 2147483648ll, "need 0 <= num_rows < 2^31");
    EPC_CHECK_ARG(num_scans >= 0 && num_scans <= (1 << 24), "need 0 <= num_scans <= 2^24");
    EPC_CHECK_ARG(num_poses >= 2 && num_poses <= (1 << 24), "need 2 <= num_poses <= 2^24");
    EPC_CHECK_ARG(max_gap_ns >= 1 && max_gap_ns < 2147483648ll, "need 1 <= max_gap_ns < 2^31");
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_deskew_workspace_bytes(num_scans, num_poses, num_rows));
    hipStream_t st = (hipStream_t)stream;
    const st_ws w = st_layout(workspace, num_scans);
    if (int rc = scan_clear_words_launch(w.head, ST_HEAD, st, __func__)) return rc;
    const int most = num_scans > num_poses ? num_scans : num_poses;
    hipLaunchKernelGGL(stamps_check_kernel, dim3(st_blocks(most)), dim3(ST_THREADS), 0, st, offsets, num_rows, num_scans, pose_time,
                       num_poses, w.head);
    EPC_CHECK_LAUNCH();
    if (num_scans > 0) {
        hipLaunchKernelGGL(stamps_scan_kernel, dim3(st_blocks(num_scans)), dim3(ST_THREADS), 0, st, scan_time, pose_time, pose, num_poses,
                           max_gap_ns, (const int32_t*)w.head, 0, num_scans, scan_pose, status, w.scan_j);
        EPC_CHECK_LAUNCH();
    }
    const int tiles = (int)((num_rows + ST_TILE - 1) / ST_TILE);
    if (point_dt && num_scans > 0 && tiles > 0) {
        hipLaunchKernelGGL(stamps_row_kernel, dim3(tiles), dim3(ST_THREADS), 0, st, points, offsets, num_scans, point_dt, scan_time,
                           pose_time, pose, num_poses, max_gap_ns, (const double*)scan_pose, (const int32_t*)w.head,
                           (const int32_t*)w.scan_j, status, points_out);
        EPC_CHECK_LAUNCH();
    }
    return EPC_OK;
}
