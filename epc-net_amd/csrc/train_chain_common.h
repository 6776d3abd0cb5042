// Device helpers shared by the launch chain (train_chain.hip) and the persistent chain (train_chain_persist.hip): tile algebra,
// the pooled training-mode BatchNorm, the moment / sum partials -- and ONE definition of each stage of the forward, from which
// chain_fwd_gather_kernel, chain_fwd_linear_kernel and the phases of chain_fwd_persist_kernel are built: ch_stage_fwd_weights,
// ch_tile_frags, ch_tile_product, act4, ch_merge_stats (the neighbour gather is neighbour_mean_of, train_common.h).  The two forms of
// the forward owe each other the same products in the same arithmetic on the same operands; they get them by calling the same code.
// See train_chain.hip's header for the design.
#pragma once
#include "train_common.h"

// Geometry.  A workgroup takes `wg_rows` consecutive rows (= one partial), a multiple of 32; its waves take the 32-row tiles
// wave, wave + nw, ... .  wg_rows is chosen on the host so that the grid is ONE workgroup per CU whenever the rows allow it
// (epc_chain_wg_rows: tiles / CUs rounded up -- 9 tiles for the 73 728 rows of an 18 x 4096 tuple on 256 CUs, 11 for 22 clouds):
// fixed 256-row workgroups were 288 on 256 CUs, i.e. 32 CUs with twice the work of the others, and these kernels are one dependent
// chain per wave -- the kernel took as long as its busiest CU.  One tile per wave where the registers allow (forward: up to 12 waves),
// otherwise strided tiles (backward: up to 8 waves).
#define CH_MAX_TILES 16      // tiles per workgroup (wg_rows <= 512)
#define CH_FWD_MAX_WAVES 8     // the row-streaming forward layer: two waves per SIMD (at three its weight fragments spill)
#define CH_GATHER_MAX_WAVES 12 // the gather layer: three waves per SIMD, one tile each -- bytes in flight are what it is short of
#define CH_BWD_MAX_WAVES 8

__device__ __forceinline__ void ch_ld8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ __forceinline__ void ch_st8(float* p, const float (&v)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ---- a training-mode BatchNorm whose batch moments come from a producer's partials (or are given) -----------------------
struct ChBn {
    const float* stats;   // partials [parts][3][64]: sums of (v - p), (v - p)^2 and the pivot p, of the product WITHOUT `bias`; null: mean / var given
    int parts;
    int part_rows;        // rows per partial (the last one shorter)
    const float* bias;    // added to the pooled mean (may be null)
    float* mean;          // pooled: written by workgroup 0;  given: read
    float* var;
    const float* gamma;
    const float* beta;
};

// Pools the partials' moments: thread (column quad cq = tid & 15, slice ps = tid >> 4) merges partials ps, ps + 16, ... around the
// pivot of its first one, the 16 slices are rebased onto slice 0's pivot and merged in order -- double precision throughout:
//   sum (v - p0) = sum (v - pw) + n (pw - p0);   sum (v - p0)^2 = sum (v - pw)^2 + 2 (pw - p0) sum (v - pw) + n (pw - p0)^2
// mean = p0 + A / rows (+ bias), population variance = B / rows - (A / rows)^2 (tf.nn.moments).  Every workgroup computes the same
// bits.  In two halves so that the caller can put its own row loads in between: ch_bn_begin requests a thread's partials in as few
// round trips as registers allow (CH_POOL_CHUNK per trip), folds them and parks the slice in `scratch` (4 * 16 * 64 doubles);
// ch_bn_finish (after the caller has ISSUED its loads) merges the slices and leaves the layer's s, t in coef[0..1][64] (LDS).  A
// pooled prologue costs ~7 us of dependent steps when written naively (scripts/time_chain.py): the affine parameters are requested
// first, the partials in one or two trips, and the rows travel under the merge.
#define CH_POOL_CHUNK 8    // moment partials per slice and round trip (24 float4 in flight per thread): 256 partials in two trips
struct ChBnRegs {          // per-thread state between the two halves (threads 0..63: the column's affine parameters / given moments)
    float gamma, beta, bias, mean, var;
};
__device__ __forceinline__ ChBnRegs ch_bn_begin(const ChBn& bn, int rows, double* scratch) {
    // 16 slices when the workgroup has 256 threads or more (the first 256 pool), fewer in the small grids of short inputs
    const int tid = threadIdx.x, cq = tid & 15, ps = tid >> 4;
    const int nslices = min((int)blockDim.x >> 4, 16);
    ChBnRegs r;
    r.gamma = r.beta = r.bias = r.mean = r.var = 0.f;
    if (tid < 64) {
        r.gamma = bn.gamma[tid], r.beta = bn.beta[tid];
        if (bn.bias) r.bias = bn.bias[tid];
        if (!bn.stats) r.mean = bn.mean[tid], r.var = bn.var[tid];
    }
    if (!bn.stats || ps >= nslices) return r;
    double N[4] = {0, 0, 0, 0}, A[4] = {0, 0, 0, 0}, B[4] = {0, 0, 0, 0}, PL[4] = {0, 0, 0, 0};
    bool first = true;
    for (int t0 = ps; t0 < bn.parts; t0 += nslices * CH_POOL_CHUNK) {
        float4 v1[CH_POOL_CHUNK], v2[CH_POOL_CHUNK], vp[CH_POOL_CHUNK];
#pragma unroll
        for (int u = 0; u < CH_POOL_CHUNK; ++u) {
            const int t = min(t0 + nslices * u, bn.parts - 1);
            const float* p = bn.stats + (size_t)t * 192 + 4 * cq;
            v1[u] = *reinterpret_cast<const float4*>(p), v2[u] = *reinterpret_cast<const float4*>(p + 64);
            vp[u] = *reinterpret_cast<const float4*>(p + 128);
        }
#pragma unroll
        for (int u = 0; u < CH_POOL_CHUNK; ++u) {
            const int t = t0 + nslices * u;
            if (t < bn.parts) {
                const double nt = (double)min(bn.part_rows, rows - t * bn.part_rows);
                const float s1[4] = {v1[u].x, v1[u].y, v1[u].z, v1[u].w}, s2[4] = {v2[u].x, v2[u].y, v2[u].z, v2[u].w},
                            pv[4] = {vp[u].x, vp[u].y, vp[u].z, vp[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (first) PL[q] = (double)pv[q];
                    const double d = (double)pv[q] - PL[q];
                    N[q] += nt;
                    A[q] += (double)s1[q] + nt * d;
                    B[q] += (double)s2[q] + 2.0 * d * (double)s1[q] + nt * d * d;
                }
                first = false;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        scratch[(0 * 16 + ps) * 64 + 4 * cq + q] = N[q];
        scratch[(1 * 16 + ps) * 64 + 4 * cq + q] = A[q];
        scratch[(2 * 16 + ps) * 64 + 4 * cq + q] = B[q];
        scratch[(3 * 16 + ps) * 64 + 4 * cq + q] = PL[q];
    }
    return r;
}
// second half: merge (when pooled), the moments to s_mean / s_var (LDS) and -- workgroup 0 -- to bn.mean / bn.var, then s, t of the
// BatchNorm (+ReLU) applied to an operand as it is loaded into coef[0..1][64].  Ends with a barrier.
__device__ __forceinline__ void ch_bn_finish(const ChBn& bn, const ChBnRegs& r, int rows, float eps, const double* scratch,
                                             float* s_mean, float* s_var, float (*coef)[64]) {
    const int tid = threadIdx.x;
    __syncthreads();   // the slices are parked (and whatever else the caller wrote to LDS before: its weight fragments)
    if (tid < 64) {
        float mean = r.mean, var = r.var;
        if (bn.stats) {
            const double p0 = scratch[(3 * 16 + 0) * 64 + tid];
            double a = scratch[(1 * 16 + 0) * 64 + tid], b = scratch[(2 * 16 + 0) * 64 + tid];
            const int nslices = min((int)blockDim.x >> 4, 16);
            for (int s = 1; s < nslices; ++s) {
                const double n = scratch[(0 * 16 + s) * 64 + tid];
                if (n > 0.0) {
                    const double as = scratch[(1 * 16 + s) * 64 + tid], bs = scratch[(2 * 16 + s) * 64 + tid];
                    const double d = scratch[(3 * 16 + s) * 64 + tid] - p0;
                    a += as + n * d;
                    b += bs + 2.0 * d * as + n * d * d;
                }
            }
            const double m1 = a / (double)rows;
            mean = (float)(p0 + m1 + (double)r.bias);
            var = (float)fmax(b / (double)rows - m1 * m1, 0.0);
            if (blockIdx.x == 0) bn.mean[tid] = mean, bn.var[tid] = var;
        }
        s_mean[tid] = mean, s_var[tid] = var;
        const BnAffine a2 = bn_affine(mean, var, r.gamma, r.beta, eps);
        coef[0][tid] = a2.s, coef[1][tid] = a2.t;
    }
    __syncthreads();
}

#define CH_POOL_CHUNK_S 16 // sum partials per slice and round trip (32 float4 in flight per thread: ONE round trip for 256 partials)
// The two column sums of a BatchNorm backward (sum dy [mask], sum dy [mask] zhat) pooled from a producer's partials
// [parts][2][64]: thread (cq, ps) adds partials ps, ps + 16, ... in double, the slices meet in order.  scratch: 2 * 16 * 64
// doubles.  Results in s_sum[2][64] (LDS); workgroup 0 also writes dbeta = sum 0, dgamma = sum 1.  Ends with a barrier.
__device__ __forceinline__ void ch_pool_sums(const float* __restrict__ psums, int parts, double* scratch, float (*s_sum)[64],
                                             float* dbeta, float* dgamma) {
    const int tid = threadIdx.x, cq = tid & 15, ps = tid >> 4;
    const int nslices = min((int)blockDim.x >> 4, 16);
    double a[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int t0 = ps; ps < nslices && t0 < parts; t0 += nslices * CH_POOL_CHUNK_S) {
        float4 v[CH_POOL_CHUNK_S][2];
#pragma unroll
        for (int u = 0; u < CH_POOL_CHUNK_S; ++u) {
            const int t = min(t0 + nslices * u, parts - 1);
            const float* p = psums + (size_t)t * 128 + 4 * cq;
            v[u][0] = *reinterpret_cast<const float4*>(p), v[u][1] = *reinterpret_cast<const float4*>(p + 64);
        }
#pragma unroll
        for (int u = 0; u < CH_POOL_CHUNK_S; ++u)
            if (t0 + nslices * u < parts) {
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    a[k][0] += (double)v[u][k].x, a[k][1] += (double)v[u][k].y, a[k][2] += (double)v[u][k].z, a[k][3] += (double)v[u][k].w;
            }
    }
    if (ps < nslices) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) scratch[(k * 16 + ps) * 64 + 4 * cq + q] = a[k][q];
    }
    __syncthreads();
    for (int o = tid; o < 128; o += blockDim.x) {   // (a 64-thread workgroup of a short input takes both sums in turn)
        const int k = o >> 6, c = o & 63;
        double t = 0.0;
        for (int s = 0; s < nslices; ++s) t += scratch[(k * 16 + s) * 64 + c];
        s_sum[k][c] = (float)t;
        if (blockIdx.x == 0) (k ? dgamma : dbeta)[c] = (float)t;
    }
    __syncthreads();
}

// The moment partial of a workgroup from its waves' (sum, sum of squares, pivot, rows): wave 0 rebases the others onto its own pivot
// in wave order (fixed order: registers, lane halves, waves) and hands the partial's [3][64] values to store(k, column, value).
//   sum (v - p0) = sum (v - pw) + n (pw - p0),  sum (v - p0)^2 = sum (v - pw)^2 + 2 (pw - p0) sum (v - pw) + n (pw - p0)^2
// sred: [waves][3][64], snrows: [waves].  WAIT: every wave first waits for its own outstanding stores (the persistent chain posts the
// partial as a signal that they are visible).  Called by every thread; contains the barrier.
template <bool WAIT, typename STORE>
__device__ __forceinline__ void ch_merge_stats(float (&s1)[2], float (&s2)[2], const float (&piv)[2], int my_rows, float (*sred)[3][64],
                                               int* snrows, int tid, STORE store) {
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        s1[nt] += __shfl_xor(s1[nt], 32);
        s2[nt] += __shfl_xor(s2[nt], 32);
    }
    if (wave > 0 && h == 0) {
        sred[wave][0][i] = s1[0], sred[wave][0][32 + i] = s1[1];
        sred[wave][1][i] = s2[0], sred[wave][1][32 + i] = s2[1];
        sred[wave][2][i] = piv[0], sred[wave][2][32 + i] = piv[1];
    }
    if (lane == 0) snrows[wave] = my_rows;
    if constexpr (WAIT) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (wave == 0 && h == 0) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int c = 32 * nt + i;
            float t1 = s1[nt], t2 = s2[nt];
            for (int w = 1; w < nw; ++w) {
                const float n_w = (float)snrows[w];
                if (n_w > 0.f) {
                    const float dp = sred[w][2][c] - piv[nt];
                    t1 += sred[w][0][c] + n_w * dp;
                    t2 += sred[w][1][c] + (2.0f * dp) * sred[w][0][c] + n_w * dp * dp;
                }
            }
            store(0, c, t1), store(1, c, t2), store(2, c, piv[nt]);
        }
    }
}
// ... stored as plain floats [3][64] at `out`: the launch chain's partial
__device__ __forceinline__ void ch_store_stats(float (&s1)[2], float (&s2)[2], const float (&piv)[2], int my_rows, float (*sred)[3][64],
                                               int* snrows, float* out) {
    ch_merge_stats<false>(s1, s2, piv, my_rows, sred, snrows, threadIdx.x, [&](int k, int c, float v) { out[k * 64 + c] = v; });
}

#define CH_STG_STRIDE 68   // floats per row of the staging tile (272 B: conflict-free float4 rows both ways)
#define CH_STG_FLOATS (32 * CH_STG_STRIDE)

// ---- the stages of the forward ---------------------------------------------------------------------------------------------
// BatchNorm + ReLU of a lane's four channels, relu(v * s + t): the forward's own expression (bn_value's, train_common.h)
__device__ __forceinline__ float4 act4(const float4& v, const float4& s, const float4& t) {
    return make_float4(fmaxf(v.x * s.x + t.x, 0.f), fmaxf(v.y * s.y + t.y, 0.f), fmaxf(v.z * s.z + t.z, 0.f), fmaxf(v.w * s.w + t.w, 0.f));
}

// A (64, 64) weight W[k = in][n = out] as the forward's B fragments: lane (n = 32 nt + i, k group h) of k-step s holds
// W[16 s + 8 h .. + 7][n], split into PF bf16 pieces -> Wf[nt][s][piece][lane] (LDS).  The caller's barrier makes them visible.
template <int PF>
__device__ __forceinline__ void ch_stage_fwd_weights(const float* W, u32x4 (*Wf)[4][PF][64], int tid) {
    for (int f = tid; f < 2 * 4 * 64; f += blockDim.x) {
        const int l = f & 63, s4 = (f >> 6) & 3, nt = f >> 8;
        const float* src = W + (size_t)(16 * s4 + 8 * (l >> 5)) * 64 + 32 * nt + (l & 31);
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)u * 64];
        bf16x8 p[PF];
        bf16_split<PF>(v, p);
#pragma unroll
        for (int pc = 0; pc < PF; ++pc) Wf[nt][s4][pc][l] = __builtin_bit_cast(u32x4, p[pc]);
    }
}

// The wave's staging tile (32 rows x 64 f32, written in the row layout) -> its A fragments: lane (row i, k group h) of k-step s takes
// channels 16 s + 8 h .. + 7 of row i, split into PF pieces.  Between two LDS waits of the one wave that owns the tile: its writes
// have landed before the reads, and the reads are in registers before the caller overwrites the tile.
template <int PF>
__device__ __forceinline__ void ch_tile_frags(const float* tile, int lane, bf16x8 (&a)[4][PF]) {
    const int i = lane & 31, h = lane >> 5;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        float v[8];
        ch_ld8(tile + i * CH_STG_STRIDE + 16 * s4 + 8 * h, v);
        bf16_split<PF>(v, a[s4]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The 64 -> 64 product of a 32-row tile (A fragments a, rows base .. base + 31) with the staged weight, and its pivot-shifted moments:
// per out tile nt, four k-steps of bf16_prod<PF> into a zeroed accumulator; take_pivot: piv[nt] = row `base` of the product, column
// 32 nt + i (acc[0] of lane i); the rows < `rows` add v - piv, (v - piv)^2 to s1, s2 in register order, v being the product WITHOUT
// the bias (the pooling adds it to the mean), and every element goes to emit(nt, r, global row, v) -- r the accumulator register, a
// constant at every call: the element's row in the tile is mfma_row(r, h), and an address formed from the lane's own row and
// mfma_row(r, 0) keeps immediate offsets.  PAST_END: the rows of the tile past the end of the tensor are emitted too -- an LDS tile
// written whole, the sums by selects and no branch (the persistent chain's phases G and M; asked to test the row in their emit
// instead, the launch kernels got the selects as well and 4 to 16 VGPRs more).
template <int PF, bool PAST_END, typename EMIT>
__device__ __forceinline__ void ch_tile_product(const bf16x8 (&a)[4][PF], const u32x4 (*Wf)[4][PF][64], int lane, int base, int rows,
                                                bool take_pivot, float (&s1)[2], float (&s2)[2], float (&piv)[2], EMIT emit) {
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            bf16x8 w[PF];
#pragma unroll
            for (int pc = 0; pc < PF; ++pc) w[pc] = __builtin_bit_cast(bf16x8, Wf[nt][s4][pc][lane]);
            acc = bf16_prod<PF>(a[s4], w, acc);
        }
        if (take_pivot) piv[nt] = __shfl(acc[0], i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = base + mfma_row(r, h);
            const float v = acc[r];
            if (rr < rows) {
                const float d = v - piv[nt];
                s1[nt] += d;
                s2[nt] += d * d;
                if constexpr (!PAST_END) emit(nt, r, rr, v);
            }
            if constexpr (PAST_END) emit(nt, r, rr, v);
        }
    }
}

struct ChBnGiven {   // a BatchNorm with known batch moments (null mean: none)
    const float *mean, *var, *gamma, *beta;
};
// The producer's column sums go through a small per-wave LDS tile, eight channels at a time (64 per-lane accumulators -- a lane
// holds ONE row's 32 channels -- would cost the kernel its second wave per SIMD): word of (quantity q, row, channel ch) below;
// a wave's 32-lane half reads 32 distinct banks (lane = (row group g, q, ch): bank = 8 q + 16 g + 8 r + ch mod 32).
#define CH_SUMT_WORDS 640
__device__ __forceinline__ int ch_sumt_word(int qn, int row, int ch) { return qn * 328 + row * 8 + (row >> 3) * 16 + ch; }
