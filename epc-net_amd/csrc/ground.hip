// Ground removal of raw scans (include/epcnet_scans.h: epcnet_ground_remove; numpy restatement in tests/ground_ref.py): a deterministic
// plane RANSAC per scan in front of the down-sampler.  The definition is float32 with every operation rounded once (contract off) and
// integer counts, so the result is the same bits on every run and equal to numpy's.
//
// The offsets are device data: every grid is sized from num_rows, B and H alone, and every kernel finds its scans itself.
//   ground_build_kernel    one workgroup per scan: validates ALL offsets (every workgroup alike: B <= 65535 words from L2), draws the
//                          vertices of its H hypotheses, writes their planes (n_x, n_y, n_z, d0, thr; thr = -1 for an invalid one, which
//                          no row can meet: the scorer needs no flag) and zeroes the scan's counters
//   ground_score_kernel    the hot path.  Flat tiles of GR_TILE rows over [0, num_rows): one 100 000-row scan is spread over ~100
//                          workgroups.  The tile's rows sit in LDS as x | y | z arrays (a non-finite row as three NaN: it never counts);
//                          LANES ARE HYPOTHESES: a wave holds the five plane words of 64 hypotheses in registers and reads the rows by
//                          broadcast (one address for all lanes, ds_read_b128 = four rows), 9 non-fused operations per (row, hypothesis).
//                          The sixteen waves take every sixteenth quad of rows; their counts meet in an LDS array (integer ds_add) and leave
//                          as ONE integer global add per (tile, scan, hypothesis).  A tile that crosses a scan boundary, or holds several
//                          tiny scans, does this once per scan it touches.  The finite rows are counted the same way.
//   ground_select_kernel   one workgroup per scan: arg-max (ties: smaller h), acceptance, plane / info / status, the chosen plane
//   ground_mark_kernel     flat tiles again: e for the chosen plane, NaN rows out; in place safe (the vertices were read in launch 1)
// Integer atomics only: order-independent, hence deterministic.
#include "scan_common.h"
#include "../../include/epcnet_scans.h"

#define GR_THREADS 256
#define GR_WAVES (GR_THREADS / 64)
#define GR_TILE 1024           // rows per scorer tile (tests/test_gpu_ground.py names it T): 12 KB of LDS
#define GS_THREADS 1024        // the scorer's workgroup: 16 waves share a tile, so that ONE tile's latency (a single scan) is short
#define GS_WAVES (GS_THREADS / 64)
#define GR_MARK_TILE 1024
#define GR_MAX_H 1024
#define GR_META 4              // per scan: begin, M, ok, offsets valid
#define GR_CHOSEN 8            // per scan: n_x n_y n_z d0 thr (float bits), accepted, 2 spare

// the workspace, in 4-byte words: meta | finite | chosen | scores | planes (per scan 5 arrays of H: n_x n_y n_z d0 thr)
struct gr_ws {
    int32_t* meta;
    int32_t* finite;
    int32_t* chosen;
    int32_t* scores;
    float* planes;
};
__host__ __device__ __forceinline__ gr_ws gr_carve(void* workspace, int B, int H) {
    gr_ws w;
    const size_t b = (size_t)(B > 0 ? B : 1);
    w.meta = reinterpret_cast<int32_t*>(workspace);
    w.finite = w.meta + b * GR_META;
    w.chosen = w.finite + b * 4;
    w.scores = w.chosen + b * GR_CHOSEN;
    w.planes = reinterpret_cast<float*>(w.scores + b * (size_t)H);
    return w;
}
__host__ __device__ __forceinline__ size_t gr_ws_words(int B, int H) {
    return (size_t)(B > 0 ? B : 1) * (GR_META + 4 + GR_CHOSEN + 6 * (size_t)H);
}

__device__ __forceinline__ float gr_dot(float nx, float ny, float nz, float x, float y, float z) {
#pragma clang fp contract(off)
    return (nx * x + ny * y) + nz * z;
}
// e(row) = ((n_x x + n_y y) + n_z z) - d0
__device__ __forceinline__ float gr_e(float nx, float ny, float nz, float d0, float x, float y, float z) {
#pragma clang fp contract(off)
    return gr_dot(nx, ny, nz, x, y, z) - d0;
}
__device__ __forceinline__ int gr_inlier(float nx, float ny, float nz, float d0, float thr, float x, float y, float z) {
#pragma clang fp contract(off)
    const float e = gr_e(nx, ny, nz, d0, x, y, z);
    return e * e <= thr ? 1 : 0;
}

// ---- launch 1: offsets, vertices, planes, zeroed counters ---------------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void ground_build_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                  int num_rows, int B, int H, int K, float t, float cos2_tilt, float max_z,
                                                                  uint32_t seed_lo, uint32_t seed_hi, gr_ws ws) {
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < B; i += GR_THREADS) mine |= offsets_rule_bad(offsets, B, num_rows, i) ? 1 : 0;      // (B >= 1: index 0 is visited)
    if (mine) atomicOr(&bad, 1);
    __syncthreads();
    const bool valid = bad == 0;
    const int begin = valid ? offsets[b] : 0;
    const int rows = valid ? offsets[b + 1] - begin : 0;
    const bool ok = valid && rows <= EPC_GROUND_MAX_ROWS;
    const int M = ok ? rows : 0;
    if (tid == 0) {
        ws.meta[b * GR_META + 0] = begin;
        ws.meta[b * GR_META + 1] = M;
        ws.meta[b * GR_META + 2] = ok ? 1 : 0;
        ws.meta[b * GR_META + 3] = valid ? 1 : 0;
        ws.finite[b] = 0;
    }
    const float* pc = points + (size_t)begin * 3;
    uint32_t s = epc_mix32(seed_lo);
    s = epc_mix32(s ^ seed_hi);
    for (int h = tid; h < H; h += GR_THREADS) {
#pragma clang fp contract(off)
        const uint32_t sh = epc_mix32(s ^ (uint32_t)h);
        float p[3][3];
        bool vertices = M > 0;
        for (int j = 0; j < 3 && vertices; ++j) {
            bool have = false;
            float bx = 0.f, by = 0.f, bz = 0.f;
            for (int k = 0; k < K; ++k) {
                const uint32_t r = (uint32_t)(((unsigned long long)epc_mix32(sh ^ (uint32_t)(K * j + k)) * (unsigned long long)M) >> 32);
                const float x = pc[3 * (size_t)r], y = pc[3 * (size_t)r + 1], z = pc[3 * (size_t)r + 2];
                if (epc_finite3(x, y, z) && (!have || z < bz)) have = true, bx = x, by = y, bz = z;
            }
            p[j][0] = bx, p[j][1] = by, p[j][2] = bz;
            vertices = have;
        }
        float nx = 0.f, ny = 0.f, nz = 0.f, d0 = 0.f, thr = -1.0f;
        if (vertices) {
            const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
            const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
            nx = uy * vz - uz * vy;
            ny = uz * vx - ux * vz;
            nz = ux * vy - uy * vx;
            const float nn = (nx * nx + ny * ny) + nz * nz;
            if (nz < 0.f) nx = -nx, ny = -ny, nz = -nz;
            d0 = gr_dot(nx, ny, nz, p[0][0], p[0][1], p[0][2]);
            const bool good = nn >= 1e-12f && nn <= 3e38f && nz * nz >= cos2_tilt * nn && d0 <= max_z * nz;
            if (good) thr = (t * t) * nn;
        }
        float* pl = ws.planes + (size_t)b * 5 * H;
        pl[h] = nx, pl[H + h] = ny, pl[2 * H + h] = nz, pl[3 * H + h] = d0, pl[4 * H + h] = thr;
        ws.scores[(size_t)b * H + h] = 0;
    }
}

// ---- launch 2: the scores -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_THREADS) void ground_score_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                  int num_rows, int B, int H, gr_ws ws) {
    __shared__ __attribute__((aligned(16))) float lx[GR_TILE];
    __shared__ __attribute__((aligned(16))) float ly[GR_TILE];
    __shared__ __attribute__((aligned(16))) float lz[GR_TILE];
    __shared__ int acc[GR_MAX_H];
    __shared__ int fin;
    if (ws.meta[3] == 0) return;                       // invalid offsets: no scan has a score (uniform: every thread reads one word)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long t0l = (long long)blockIdx.x * GR_TILE;
    const int t0 = (int)t0l;
    const int t1 = (int)(t0l + GR_TILE < (long long)num_rows ? t0l + GR_TILE : (long long)num_rows);
    const float nan = epc_nan_f32();
    for (int i = tid; i < GR_TILE; i += GS_THREADS) {
        float x = nan, y = nan, z = nan;
        if (t0 + i < t1) {
            const float* p = points + (size_t)(t0 + i) * 3;
            x = p[0], y = p[1], z = p[2];
            if (!epc_finite3(x, y, z)) x = y = z = nan;
        }
        lx[i] = x, ly[i] = y, lz[i] = z;
    }
    for (int h = tid; h < H; h += GS_THREADS) acc[h] = 0;
    if (tid == 0) fin = 0;
    __syncthreads();

    const int groups = H >> 6;
    for (int b = first_scan_behind(offsets, 0, B, t0); b < B; ++b) {
        const int begin = offsets[b], end = offsets[b + 1];
        if (begin >= t1) break;
        if (ws.meta[b * GR_META + 2] == 0) continue;   // a scan of more than 2^20 rows: failed alone
        const int r0 = (begin > t0 ? begin : t0) - t0, r1 = (end < t1 ? end : t1) - t0;      // the segment, tile-local
        if (r1 <= r0) continue;
        // finite rows of the segment
        {
            int c = 0;
            for (int i = r0 + tid; i < r1; i += GS_THREADS) c += lx[i] == lx[i] ? 1 : 0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0 && c) atomicAdd(&fin, c);
        }
        // the quads of rows that lie wholly inside the segment, every sixteenth one for this wave: read by broadcast (one address in all
        // lanes), the next quad fetched while this one is scored; the at most six rows in front of and behind them go to wave 0
        const int qa = (r0 + 3) >> 2, qb = r1 >> 2;
        const int qs = qa + ((wave - qa) & (GS_WAVES - 1));
        const int head_end = r1 < (qa << 2) ? r1 : (qa << 2);
        const int tail_begin = head_end > (qb << 2) ? head_end : (qb << 2);
        const float* pl = ws.planes + (size_t)b * 5 * H;
        for (int g = 0; g < groups; ++g) {
            const int h = g * 64 + lane;
            const float nx = pl[h], ny = pl[H + h], nz = pl[2 * H + h], d0 = pl[3 * H + h], thr = pl[4 * H + h];
            int cnt = 0;
            if (qs < qb) {
                float4 X = *reinterpret_cast<const float4*>(&lx[qs << 2]);
                float4 Y = *reinterpret_cast<const float4*>(&ly[qs << 2]);
                float4 Z = *reinterpret_cast<const float4*>(&lz[qs << 2]);
                for (int q = qs; q < qb; q += GS_WAVES) {
                    const int qn = q + GS_WAVES < GR_TILE / 4 ? q + GS_WAVES : q;      // (inside the arrays; unused behind the last quad)
                    const float4 Xn = *reinterpret_cast<const float4*>(&lx[qn << 2]);
                    const float4 Yn = *reinterpret_cast<const float4*>(&ly[qn << 2]);
                    const float4 Zn = *reinterpret_cast<const float4*>(&lz[qn << 2]);
                    cnt += gr_inlier(nx, ny, nz, d0, thr, X.x, Y.x, Z.x);
                    cnt += gr_inlier(nx, ny, nz, d0, thr, X.y, Y.y, Z.y);
                    cnt += gr_inlier(nx, ny, nz, d0, thr, X.z, Y.z, Z.z);
                    cnt += gr_inlier(nx, ny, nz, d0, thr, X.w, Y.w, Z.w);
                    X = Xn, Y = Yn, Z = Zn;
                }
            }
            if (wave == 0) {
                for (int i = r0; i < head_end; ++i) cnt += gr_inlier(nx, ny, nz, d0, thr, lx[i], ly[i], lz[i]);
                for (int i = tail_begin; i < r1; ++i) cnt += gr_inlier(nx, ny, nz, d0, thr, lx[i], ly[i], lz[i]);
            }
            if (cnt) atomicAdd(&acc[h], cnt);
        }
        __syncthreads();
        for (int h = tid; h < H; h += GS_THREADS) {
            const int v = acc[h];
            if (v) {
                atomicAdd(&ws.scores[(size_t)b * H + h], v);
                acc[h] = 0;
            }
        }
        if (tid == 0) {
            if (fin) atomicAdd(&ws.finite[b], fin);
            fin = 0;
        }
        __syncthreads();
    }
}

// ---- launch 3: the choice -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void ground_select_kernel(int H, float min_share, gr_ws ws, float* __restrict__ plane,
                                                                   int32_t* __restrict__ info, int32_t* __restrict__ status) {
    __shared__ unsigned long long best_w[GR_WAVES];
    __shared__ int valid_w[GR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pl = ws.planes + (size_t)b * 5 * H;
    // (score << 32) | (0xffffffff - h): the largest score, then the smallest h; 0 = no valid hypothesis (a valid one is >= 2^32 - H > 0)
    unsigned long long best = 0ull;
    int nvalid = 0;
    for (int h = tid; h < H; h += GR_THREADS)
        if (pl[4 * H + h] >= 0.f) {
            ++nvalid;
            const unsigned long long v = ((unsigned long long)(uint32_t)ws.scores[(size_t)b * H + h] << 32) | (0xffffffffu - (uint32_t)h);
            best = v > best ? v : best;
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
        nvalid += __shfl_xor(nvalid, off);
    }
    if (lane == 0) best_w[wave] = best, valid_w[wave] = nvalid;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < GR_WAVES; ++w) best = best_w[w] > best ? best_w[w] : best, nvalid += valid_w[w];
    const bool ok = ws.meta[b * GR_META + 2] != 0;
    const int finite = ws.finite[b];
    const int hbest = best ? (int)(0xffffffffu - (uint32_t)best) : -1;
    const int score = (int)(best >> 32);
    bool accepted = false;
    if (ok && hbest >= 0) {
#pragma clang fp contract(off)
        accepted = score >= 3 && (float)score >= min_share * (float)finite;
    }
    const float nan = epc_nan_f32();
    float w[5] = {nan, nan, nan, nan, -1.0f};
    if (accepted)
#pragma unroll
        for (int c = 0; c < 5; ++c) w[c] = pl[c * H + hbest];
#pragma unroll
    for (int c = 0; c < 4; ++c) plane[(size_t)b * 4 + c] = w[c];
#pragma unroll
    for (int c = 0; c < 5; ++c) ws.chosen[b * GR_CHOSEN + c] = __float_as_int(w[c]);
    ws.chosen[b * GR_CHOSEN + 5] = accepted ? 1 : 0;
    status[b] = accepted ? 0 : EPC_STATUS_NO_GROUND;
    if (info) {
        info[(size_t)b * 4 + 0] = ok ? finite : 0;
        info[(size_t)b * 4 + 1] = ok ? nvalid : 0;
        info[(size_t)b * 4 + 2] = ok ? hbest : 0;
        info[(size_t)b * 4 + 3] = ok ? score : 0;
    }
}

// ---- launch 4: the rows -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gr_copy_rows(const float* __restrict__ points, float* __restrict__ out, int r0, int r1) {
    if (out == points) return;
    for (int r = r0 + (int)threadIdx.x; r < r1; r += GR_THREADS) {
        const size_t o = (size_t)r * 3;
        const float x = points[o], y = points[o + 1], z = points[o + 2];
        out[o] = x, out[o + 1] = y, out[o + 2] = z;
    }
}
// no __restrict__ on the rows: points_out may be points (every row is read and written by one thread)
__global__ __launch_bounds__(GR_THREADS) void ground_mark_kernel(const float* points, const int32_t* __restrict__ offsets, int num_rows,
                                                                 int B, gr_ws ws, float* out) {
    const long long t0l = (long long)blockIdx.x * GR_MARK_TILE;
    const int t0 = (int)t0l;
    const int t1 = (int)(t0l + GR_MARK_TILE < (long long)num_rows ? t0l + GR_MARK_TILE : (long long)num_rows);
    if (ws.meta[3] == 0) {                             // invalid offsets: every row is copied
        gr_copy_rows(points, out, t0, t1);
        return;
    }
    const float nan = epc_nan_f32();
    int cur = t0;
    for (int b = first_scan_behind(offsets, 0, B, t0); b < B; ++b) {
        const int begin = offsets[b], end = offsets[b + 1];
        if (begin >= t1) break;
        const int r0 = begin > cur ? begin : cur, r1 = end < t1 ? end : t1;
        if (r1 <= r0) continue;
        gr_copy_rows(points, out, cur, r0);            // rows inside no scan
        if (ws.chosen[b * GR_CHOSEN + 5] == 0) {
            gr_copy_rows(points, out, r0, r1);
        } else {
            const int32_t* c = ws.chosen + b * GR_CHOSEN;
            const float nx = __int_as_float(c[0]), ny = __int_as_float(c[1]), nz = __int_as_float(c[2]), d0 = __int_as_float(c[3]),
                        thr = __int_as_float(c[4]);
            for (int r = r0 + (int)threadIdx.x; r < r1; r += GR_THREADS) {
#pragma clang fp contract(off)
                const size_t o = (size_t)r * 3;
                const float x = points[o], y = points[o + 1], z = points[o + 2];
                const float e = gr_e(nx, ny, nz, d0, x, y, z);
                const bool gone = epc_finite3(x, y, z) && (e < 0.f || e * e <= thr);
                if (gone)
                    out[o] = nan, out[o + 1] = nan, out[o + 2] = nan;
                else if (out != points)
                    out[o] = x, out[o + 1] = y, out[o + 2] = z;
            }
        }
        cur = r1;
    }
    gr_copy_rows(points, out, cur, t1);
}

static bool gr_supported(int num_clouds, int hypotheses, long long num_rows) {
    return num_clouds >= 0 && num_clouds <= 65535 && hypotheses >= 64 && hypotheses <= GR_MAX_H && hypotheses % 64 == 0 && num_rows >= 0 &&
           num_rows <= 2147483647ll;
}

extern "C" size_t epcnet_ground_workspace_bytes(int num_clouds, int hypotheses, long long num_rows) {
    if (!gr_supported(num_clouds, hypotheses, num_rows)) return 0;
    return gr_ws_words(num_clouds, hypotheses) * sizeof(int32_t);
}

extern "C" int epcnet_ground_remove(const float* points, const int32_t* offsets, int num_rows, int num_clouds, int hypotheses, int draws,
                                    float threshold, float cos2_tilt, float max_z, float min_share, long long seed, float* points_out,
                                    float* plane, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG(points && offsets && points_out && workspace && (num_clouds == 0 || (plane && status)), "null pointer");
    EPC_CHECK_ARG(num_rows >= 0, "num_rows must not be negative");
    EPC_CHECK_ARG(num_clouds >= 0 && num_clouds <= 65535, "need 0 <= num_clouds <= 65535");
    EPC_CHECK_ARG(hypotheses >= 64 && hypotheses <= GR_MAX_H && hypotheses % 64 == 0, "hypotheses must be a multiple of 64 in [64, 1024]");
    EPC_CHECK_ARG(draws >= 1 && draws <= 16, "draws must be in [1, 16]");
    EPC_CHECK_ARG(__builtin_isfinite(threshold) && threshold > 0.f, "threshold must be finite and > 0");
    EPC_CHECK_ARG(cos2_tilt > 0.f && cos2_tilt <= 1.f, "cos2_tilt must be in (0, 1]");
    EPC_CHECK_ARG(max_z == max_z, "max_z must not be NaN (+Inf: no limit)");
    EPC_CHECK_ARG(min_share >= 0.f && min_share <= 1.f, "min_share must be in [0, 1]");
    EPC_CHECK_WORKSPACE(workspace, workspace_bytes, epcnet_ground_workspace_bytes(num_clouds, hypotheses, num_rows));
    hipStream_t st = (hipStream_t)stream;
    if (num_clouds == 0) {                             // no scan: every row lies inside none
        if (points_out != points && num_rows > 0 &&
            hipMemcpyAsync(points_out, points, (size_t)num_rows * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            epc_set_error("epcnet_ground_remove: copy failed");
            return EPC_EHIP;
        }
        return EPC_OK;
    }
    const gr_ws ws = gr_carve(workspace, num_clouds, hypotheses);
    const uint32_t seed_lo = (uint32_t)(unsigned long long)seed, seed_hi = (uint32_t)((unsigned long long)seed >> 32);
    const int tiles = (int)(((long long)num_rows + GR_TILE - 1) / GR_TILE);
    const int mark_tiles = (int)(((long long)num_rows + GR_MARK_TILE - 1) / GR_MARK_TILE);
    hipLaunchKernelGGL(ground_build_kernel, dim3(num_clouds), dim3(GR_THREADS), 0, st, points, offsets, num_rows, num_clouds, hypotheses,
                       draws, threshold, cos2_tilt, max_z, seed_lo, seed_hi, ws);
    EPC_CHECK_LAUNCH();
    if (tiles > 0) {
        hipLaunchKernelGGL(ground_score_kernel, dim3(tiles), dim3(GS_THREADS), 0, st, points, offsets, num_rows, num_clouds, hypotheses, ws);
        EPC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ground_select_kernel, dim3(num_clouds), dim3(GR_THREADS), 0, st, hypotheses, min_share, ws, plane, info, status);
    EPC_CHECK_LAUNCH();
    if (mark_tiles > 0) {
        hipLaunchKernelGGL(ground_mark_kernel, dim3(mark_tiles), dim3(GR_THREADS), 0, st, points, offsets, num_rows, num_clouds, ws,
                           points_out);
        EPC_CHECK_LAUNCH();
    }
    return EPC_OK;
}
