// Grid-average down-sampling of raw scans to exactly N points per cloud (include/epcnet.h: epc_grid_downsample) -- the stage in
// front of the sort for clouds that are not already N-point benchmark files.  The definition (header comment; numpy restatement in
// tests/downsample_ref.py) is integer arithmetic behind the quantisation, so the result is the same bits on every run and equal to
// numpy's.
//
// One workgroup (1024 threads) per cloud, the cloud's working set in LDS, the points re-read from global memory (L2) once per pass:
//   pass 1            finite points, bounding box
//   probes            "are there >= N distinct cells at R?" for R = 1024 and the ~10 R of the bisection: a key-only open-addressing
//                     table (LDS atomicCAS), the pass stops once N distinct keys are in -- a probe above R* ends after a fraction of
//                     the points
//   pass at R*        the same table with a count per slot (stops at 2N + 1 keys: the cloud fails)
//   in LDS            table -> (key << 32 | count) array (staged through registers, the array aliases the table), bitonic sort by key,
//                     threshold count c* of the selection by bisection, ordered scans -> the N kept cells in key order
//   pass at R*        u32 sums of the in-cell fractions of the kept cells (binary search of the point's key among the N kept keys)
//   output            q = cell * 4096 + sum / count per axis, then the chosen normalisation
// LDS (dynamic) for table size T = pow2 >= 4N (>= 4096):  [0, 4T) keys | [4T, 8T) counts;  afterwards  [0, 8 * np2 <= 4T) sorted pairs,
// [4T, 4T + 20N) kept keys, kept counts, three sums.  N = 4096: 144 KB of the CU's 160 KB.
// Integer LDS atomics only: order-independent, hence deterministic.  Every float operation of the quantisation and of the output is
// rounded once (contract off; the division is hipcc's default correctly rounded one).
#include "scan_common.h"

#define GD_THREADS 1024
#define GD_WAVES (GD_THREADS / 64)
#define GD_MIN_N 32
#define GD_MAX_N 4096
#define GD_MAX_M (1 << 20)
#define GD_EMPTY 0xffffffffu
#define GD_MIN_TABLE 4096      // > the largest stop limit of a small N (2 * 32 + 1) plus one insert in flight per thread
#define GD_WS_WORDS 8          // workspace words per cloud: finite points, R*, D(R*), last kept count, lo x y z, e (float bits)

__host__ __device__ __forceinline__ int gd_table_slots(int n) {
    int t = GD_MIN_TABLE;
    while (t < 4 * n) t <<= 1;
    return t;
}
__host__ __device__ __forceinline__ size_t gd_lds_bytes(int n) {
    const size_t t = (size_t)gd_table_slots(n);
    const size_t a = 8 * t, b = 4 * t + 20 * (size_t)n;
    return a > b ? a : b;
}

struct gd_scratch {            // static LDS: block reductions, the probes' distinct-key counter
    float f[6][GD_WAVES];
    long long l[3][GD_WAVES];
    int i[GD_WAVES];
    int distinct;
};

// the point's three coordinates as dwords (rows are 12 bytes and a cloud may start at any row: no 16-byte alignment)
__device__ __forceinline__ bool gd_load(const float* __restrict__ pc, int j, float& x, float& y, float& z) {
    x = pc[3 * j], y = pc[3 * j + 1], z = pc[3 * j + 2];
    return epc_finite3(x, y, z);
}

// u = min((int)(((p - lo) * s) * 4096), R * 4096 - 1) per axis, each operation rounded once
__device__ __forceinline__ void gd_quantise(float x, float y, float z, float lox, float loy, float loz, float s, int umax, int& ux,
                                            int& uy, int& uz) {
#pragma clang fp contract(off)
    const float tx = (x - lox) * s, ty = (y - loy) * s, tz = (z - loz) * s;
    ux = min((int)(tx * 4096.0f), umax);
    uy = min((int)(ty * 4096.0f), umax);
    uz = min((int)(tz * 4096.0f), umax);
}
__device__ __forceinline__ unsigned gd_key(int ux, int uy, int uz) {
    return ((unsigned)(uz >> 12) * 1024u + (unsigned)(uy >> 12)) * 1024u + (unsigned)(ux >> 12);
}
__device__ __forceinline__ float gd_scale(int R, float e) {
#pragma clang fp contract(off)
    return (float)R / e;
}

// Slot of `key` in the open-addressing table (linear probing), inserted when absent: created = this call made the entry.  -1 when
// the table has no room (cannot happen under the stop limits: see GD_MIN_TABLE; the bound keeps the loop finite regardless).
__device__ __forceinline__ int gd_insert(unsigned* tab, unsigned mask, int shift, unsigned key, bool& created) {
    unsigned h = (key * 2654435761u) >> shift;
    created = false;
    for (unsigned it = 0; it <= mask; ++it) {
        const unsigned cur = tab[h];
        if (cur == key) return (int)h;
        if (cur == GD_EMPTY) {
            const unsigned old = atomicCAS(&tab[h], GD_EMPTY, key);
            if (old == GD_EMPTY) {
                created = true;
                return (int)h;
            }
            if (old == key) return (int)h;
        }
        h = (h + 1) & mask;
    }
    return -1;
}

__device__ __forceinline__ int gd_block_sum(int v, int* slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();           // the previous reduction's readers are done with `slot`
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < GD_WAVES; ++w) t += slot[w];
    return t;
}
__device__ __forceinline__ int gd_block_max(int v, int* slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = slot[0];
#pragma unroll
    for (int w = 1; w < GD_WAVES; ++w) t = max(t, slot[w]);
    return t;
}
// D(R) >= limit?  Key-only table; the pass stops once `limit` distinct keys are in.  With counts != nullptr every point also adds
// one to its key's count (the pass at R*).  Returns the number of distinct keys seen, exact when below `limit`.
__device__ __forceinline__ int gd_probe(const float* __restrict__ pc, int M, float lox, float loy, float loz, float e, int R, int limit,
                                        unsigned* tab, unsigned* counts, int T, int shift, gd_scratch& sc) {
    const int tid = threadIdx.x;
    for (int i = tid; i < T; i += GD_THREADS) {
        tab[i] = GD_EMPTY;
        if (counts) counts[i] = 0u;
    }
    if (tid == 0) sc.distinct = 0;
    __syncthreads();
    const float s = gd_scale(R, e);
    const int umax = R * 4096 - 1;
    for (int j = tid; j < M; j += GD_THREADS) {
        if (__hip_atomic_load(&sc.distinct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= limit) break;
        float x, y, z;
        if (!gd_load(pc, j, x, y, z)) continue;
        int ux, uy, uz;
        gd_quantise(x, y, z, lox, loy, loz, s, umax, ux, uy, uz);
        bool created;
        const int slot = gd_insert(tab, (unsigned)T - 1u, shift, gd_key(ux, uy, uz), created);
        if (created) atomicAdd(&sc.distinct, 1);
        if (counts && slot >= 0) atomicAdd(&counts[slot], 1u);
    }
    __syncthreads();
    const int d = sc.distinct;
    __syncthreads();           // everybody has read it before the next probe resets it
    return d;
}

__global__ __launch_bounds__(GD_THREADS) void grid_downsample_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                     int N, int normalize, float* __restrict__ xyz_out,
                                                                     int32_t* __restrict__ status, int32_t* __restrict__ info,
                                                                     int32_t* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gd_lds[];
    __shared__ gd_scratch sc;
    const int cloud = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = gd_table_slots(N);
    const int shift = 32 - (31 - __clz(T));
    unsigned* tab = reinterpret_cast<unsigned*>(gd_lds);
    unsigned* tcount = tab + T;
    float* out = xyz_out + (size_t)cloud * N * 3;

    // a cloud the offsets describe wrongly (decreasing, negative, more than 2^20 points) is a failed cloud: device data, device check
    const int begin = offsets[cloud], end = offsets[cloud + 1];
    const bool described = begin >= 0 && end >= begin && end - begin <= GD_MAX_M;
    const int M = described ? end - begin : 0;
    const float* pc = points + (size_t)(described ? begin : 0) * 3;

    int words[4] = {0, 0, 0, 0};           // finite points, R*, D(R*), count of the last kept cell
    float lox = 0.f, loy = 0.f, loz = 0.f, e = 0.f;
    bool ok = true;

    // ---- pass 1: finite points and their bounding box ----------------------------------------------------------------------------
    {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        int nf = 0;
        for (int j = tid; j < M; j += GD_THREADS) {
            float x, y, z;
            if (!gd_load(pc, j, x, y, z)) continue;
            ++nf;
            lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                lo[d] = fminf(lo[d], __shfl_xor(lo[d], off));
                hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off));
            }
            if (lane == 0) sc.f[d][wave] = lo[d], sc.f[3 + d][wave] = hi[d];
        }
        words[0] = gd_block_sum(nf, sc.i);            // (its barriers publish sc.f as well)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = sc.f[d][0], hi[d] = sc.f[3 + d][0];
#pragma unroll
            for (int w = 1; w < GD_WAVES; ++w) lo[d] = fminf(lo[d], sc.f[d][w]), hi[d] = fmaxf(hi[d], sc.f[3 + d][w]);
        }
        lox = lo[0], loy = lo[1], loz = lo[2];
        if (words[0] > 0) e = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
        // e == 0: all points identical.  An extent or a finest-grid scale that is not finite quantises every point to one of two
        // values per axis (<= 8 cells < N): the same failure by the definition, decided here without converting an Inf to int
        ok = words[0] >= N && e > 0.f && __builtin_isfinite(e) && __builtin_isfinite(gd_scale(1024, e));
    }

    // ---- the resolution: D(1024) >= N, then the bisection (the definition: D is not monotone) ------------------------------------
    int Rs = 1024, D = 0;
    if (ok) ok = gd_probe(pc, M, lox, loy, loz, e, 1024, N, tab, nullptr, T, shift, sc) >= N;
    if (ok) {
        int a = 1, b = 1024;
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (gd_probe(pc, M, lox, loy, loz, e, m, N, tab, nullptr, T, shift, sc) >= N)
                b = m;
            else
                a = m;
        }
        Rs = b;
        // ---- pass at R*: every key and its count; more than 2N cells fail the cloud (the word then says 2N + 1) -------------------
        D = gd_probe(pc, M, lox, loy, loz, e, Rs, 2 * N + 1, tab, tcount, T, shift, sc);
        words[1] = Rs;
        words[2] = min(D, 2 * N + 1);
        ok = D <= 2 * N;
    }

    if (ok) {
        // ---- table -> (key << 32 | count), sorted by key ----------------------------------------------------------------------------
        unsigned long long* pairs = reinterpret_cast<unsigned long long*>(gd_lds);
        int np2 = 32;
        while (np2 < D) np2 <<= 1;
        {
            const int spt = T / GD_THREADS;        // 4, 8 or 16 consecutive slots per thread, staged in registers: pairs aliases tab
            unsigned k[16], c[16];
            int mine = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                k[r] = GD_EMPTY, c[r] = 0u;
                if (r < spt) {
                    k[r] = tab[tid * spt + r], c[r] = tcount[tid * spt + r];
                    mine += k[r] != GD_EMPTY ? 1 : 0;
                }
            }
            int total;
            int at = block_scan<GD_WAVES>(mine, sc.i, total);   // (its barriers: every slot has been read before any pair is written)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (k[r] != GD_EMPTY) pairs[at++] = ((unsigned long long)k[r] << 32) | c[r];
            for (int i = D + tid; i < np2; i += GD_THREADS) pairs[i] = ~0ull;
            __syncthreads();
        }
        for (int k = 2; k <= np2; k <<= 1)
            for (int s = k >> 1; s > 0; s >>= 1) {
                for (int t = tid; t < np2 / 2; t += GD_THREADS) {
                    const int i0 = ((t & ~(s - 1)) << 1) | (t & (s - 1)), i1 = i0 + s;     // (s is a power of two)
                    const bool up = (i0 & k) == 0;
                    const unsigned long long p0 = pairs[i0], p1 = pairs[i1];
                    if ((p0 > p1) == up) pairs[i0] = p1, pairs[i1] = p0;
                }
                __syncthreads();
            }

        // ---- selection: the N cells first in (count descending, key ascending) -------------------------------------------------------
        // c* = the largest c with #{count >= c} >= N (bisection on c); cells above c* are kept, of those AT c* the first
        // N - #{count > c*} in key order.
        const int per = (np2 + GD_THREADS - 1) / GD_THREADS;      // 1, 2, 4 or 8 consecutive pairs per thread
        unsigned cnt[8];
        int cmax = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = tid * per + r;
            cnt[r] = (r < per && i < D) ? (unsigned)pairs[i] : 0u;
            cmax = max(cmax, (int)cnt[r]);
        }
        cmax = gd_block_max(cmax, sc.i);
        int ca = 1, cb = cmax + 1;             // #{count >= ca} = D >= N; #{count >= cb} = 0
        while (cb - ca > 1) {
            const int cm = (ca + cb) >> 1;
            int g = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) g += cnt[r] >= (unsigned)cm ? 1 : 0;
            if (gd_block_sum(g, sc.i) >= N)
                ca = cm;
            else
                cb = cm;
        }
        const unsigned cstar = (unsigned)ca;
        int above = 0, equal = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) above += cnt[r] > cstar ? 1 : 0, equal += cnt[r] == cstar ? 1 : 0;
        const int ties_kept = N - gd_block_sum(above, sc.i);
        int unused;
        int tie_rank = block_scan<GD_WAVES>(equal, sc.i, unused);
        int kept = 0;
        unsigned keep_mask = 0u;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool k = cnt[r] > cstar || (cnt[r] == cstar && tie_rank < ties_kept);
            tie_rank += cnt[r] == cstar ? 1 : 0;
            keep_mask |= k ? 1u << r : 0u;
            kept += k ? 1 : 0;
        }
        int at = block_scan<GD_WAVES>(kept, sc.i, unused);
        unsigned* kkey = tab + T;              // the N kept keys in ascending order, their counts, the three sums
        unsigned* kcnt = kkey + N;
        unsigned* ksum = kcnt + N;
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (keep_mask >> r & 1u) {
                kkey[at] = (unsigned)(pairs[tid * per + r] >> 32);
                kcnt[at] = cnt[r];
                ++at;
            }
        for (int i = tid; i < 3 * N; i += GD_THREADS) ksum[i] = 0u;
        words[3] = (int)cstar;
        __syncthreads();

        // ---- pass at R*: sums of the in-cell fractions of the kept cells ------------------------------------------------------------
        {
            const float s = gd_scale(Rs, e);
            const int umax = Rs * 4096 - 1;
            for (int j = tid; j < M; j += GD_THREADS) {
                float x, y, z;
                if (!gd_load(pc, j, x, y, z)) continue;
                int ux, uy, uz;
                gd_quantise(x, y, z, lox, loy, loz, s, umax, ux, uy, uz);
                const unsigned key = gd_key(ux, uy, uz);
                int l = 0, h = N;              // lower bound of key among the kept keys
                while (l < h) {
                    const int m = (l + h) >> 1;
                    if (kkey[m] < key)
                        l = m + 1;
                    else
                        h = m;
                }
                if (l < N && kkey[l] == key) {
                    atomicAdd(&ksum[l], (unsigned)(ux & 4095));
                    atomicAdd(&ksum[N + l], (unsigned)(uy & 4095));
                    atomicAdd(&ksum[2 * N + l], (unsigned)(uz & 4095));
                }
            }
            __syncthreads();
        }

        // ---- output ----------------------------------------------------------------------------------------------------------------
        int q[GD_MAX_N / GD_THREADS][3];
        long long sum[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < GD_MAX_N / GD_THREADS; ++r) {
            const int j = tid + r * GD_THREADS;
            q[r][0] = q[r][1] = q[r][2] = 0;
            if (j < N) {
                const unsigned key = kkey[j], n = kcnt[j];
                q[r][0] = (int)((key & 1023u) * 4096u + ksum[j] / n);
                q[r][1] = (int)(((key >> 10) & 1023u) * 4096u + ksum[N + j] / n);
                q[r][2] = (int)((key >> 20) * 4096u + ksum[2 * N + j] / n);
#pragma unroll
                for (int d = 0; d < 3; ++d) sum[d] += q[r][d];
            }
        }
        if (normalize) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) sum[d] += __shfl_xor(sum[d], off);
                if (lane == 0) sc.l[d][wave] = sum[d];
            }
            __syncthreads();
            int qm[3], dmax = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                long long t = 0;
#pragma unroll
                for (int w = 0; w < GD_WAVES; ++w) t += sc.l[d][w];
                qm[d] = (int)(t / N);
            }
#pragma unroll
            for (int r = 0; r < GD_MAX_N / GD_THREADS; ++r)
                if (tid + r * GD_THREADS < N)
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        q[r][d] -= qm[d];
                        dmax = max(dmax, abs(q[r][d]));
                    }
            dmax = gd_block_max(dmax, sc.i);
            {
#pragma clang fp contract(off)
                const float inv = 1.0f / (float)dmax;
#pragma unroll
                for (int r = 0; r < GD_MAX_N / GD_THREADS; ++r) {
                    const int j = tid + r * GD_THREADS;
                    if (j < N)
#pragma unroll
                        for (int d = 0; d < 3; ++d) out[3 * j + d] = (float)q[r][d] * inv;
                }
            }
        } else {
#pragma clang fp contract(off)
            const float cell = e / (float)(Rs * 4096);
            const float lo[3] = {lox, loy, loz};
#pragma unroll
            for (int r = 0; r < GD_MAX_N / GD_THREADS; ++r) {
                const int j = tid + r * GD_THREADS;
                if (j < N)
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float scaled = (float)q[r][d] * cell;
                        out[3 * j + d] = lo[d] + scaled;
                    }
            }
        }
    } else {
        const float nan = epc_nan_f32();
        for (int i = tid; i < 3 * N; i += GD_THREADS) out[i] = nan;
    }

    if (tid == 0) {
        status[cloud] = ok ? 0 : EPC_STATUS_NO_GRID;
        int32_t* f = frames + (size_t)cloud * GD_WS_WORDS;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            f[w] = words[w];
            if (info) info[(size_t)cloud * 4 + w] = words[w];
        }
        f[4] = __float_as_int(lox), f[5] = __float_as_int(loy), f[6] = __float_as_int(loz), f[7] = __float_as_int(e);
    }
}

extern "C" size_t epc_grid_downsample_workspace_bytes(int num_clouds, int n) {
    if (num_clouds < 0 || n < GD_MIN_N || n > GD_MAX_N || n % 32 != 0) return 0;
    return (size_t)(num_clouds > 0 ? num_clouds : 1) * GD_WS_WORDS * sizeof(int32_t);
}

extern "C" int epc_grid_downsample(const float* points, const int32_t* offsets, int num_clouds, int n, int normalize, float* xyz_out,
                                   int32_t* status, int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && xyz_out && status && workspace, "null pointer");
    EPC_CHECK_ARG(num_clouds >= 0, "num_clouds must not be negative");
    EPC_CHECK_ARG(n >= GD_MIN_N && n <= GD_MAX_N && n % 32 == 0, "n must be a multiple of 32 in [32, 4096]");
    EPC_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "workspace must be 4-byte aligned");
    EPC_CHECK_WORKSPACE_BYTES(workspace_bytes, epc_grid_downsample_workspace_bytes(num_clouds, n));
    if (num_clouds == 0) return EPC_OK;
    const size_t lds_bytes = gd_lds_bytes(n);
    if (int rc = epc_set_dyn_lds(reinterpret_cast<const void*>(grid_downsample_kernel), lds_bytes, "epc_grid_downsample")) return rc;
    hipLaunchKernelGGL(grid_downsample_kernel, dim3(num_clouds), dim3(GD_THREADS), lds_bytes, (hipStream_t)stream, points, offsets, n,
                       normalize ? 1 : 0, xyz_out, status, info, reinterpret_cast<int32_t*>(workspace));
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
