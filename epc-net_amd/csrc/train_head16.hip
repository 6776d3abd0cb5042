// The head of the training step -- conv5, the per-point l2 norm, the VLAD soft assignment and aggregation (models/epc-net.py:136-148,
// loupe.py:249-291), forward and backward -- with its (rows, 1024) tensors STORED AS bf16 (params["TRAIN_PRECISION"] = "bf16",
// BASELINE.json configs[2]): f32 accumulators, f32 batch statistics, f32 master weights; one bf16 value per GEMM operand.
//
// Why a file of its own: at 18 x 4096 rows the (rows, 1024) tensors are 302 MB each in f32 and the generic tile GEMM moved them ~13 times
// per step, every product re-reading and re-splitting f32 operand tiles (conv5's forward: 196 us for 15 us of matrix work).  Here every
// kernel is ONE streaming pass over bf16 rows with the small operand resident or streamed through LDS, and the feature map
// f = l2_normalize(relu(bn(z5))) is never written: BatchNorm + ReLU are applied to z5 as it is loaded (the row norm rn is a row factor
// that moves to the other operand or to the epilogue).  Their floors are byte times (189-453 MB per launch at the 5.5 TB/s a streaming
// pass reaches); they run at 0.5-1.0 of them -- LDS fragment reads, MFMA issue and the epilogue's vector work, each below the byte time,
// add up inside a wave instead of overlapping ("Training step": what bounds them, and what was tried).
//
//   tensors:  cat (rows, 256): the backbone's output, f32 and -- written beside it by the chain -- a bf16 copy, which is what these
//             kernels read;  z5 (rows, 1024) bf16 = bf16(cat16 W5_16 + b5);
//             rn (rows) f32;  za, a, dz, da (rows, 64) f32;  du / dz5 (rows, 1024) bf16 (in place);  dcat (rows, 256) f32.
//   rounding points (restated by oracle/epcnet_oracle_torch.py: _Head16): operands of every product to bf16 once; z5, du and dz5 to
//             bf16 as they are stored; batch statistics and column sums from the f32 values BEFORE that rounding.
//
//   forward   h16_conv5_fwd      z5 = bf16(cat W5 + b5), batch moments of conv5 from the accumulators            (epc-net.py:136-139)
//             hx_rowgemm<2,X>    u = relu(bn(z5)); rn = rsqrt(max(sum u^2, 1e-12)); za = rn (u Wc), moments      (:147-148, loupe.py:255)
//             (epc_assign_softmax_fwd, train_ops.hip: a = softmax(bn(za)), a_sum)                                   (loupe.py:257-276)
//             hx_colgemm         vlad[b] = u[b]^T (rn a)[b]                                                         (loupe.py:286-291)
//   backward  hx_rowgemm<2,X>    da = rn (u dvlad[b])
//             (epc_assign_softmax_bwd: dz, the cluster BatchNorm's gradients, t_row)
//             hx_colgemm         dWc = u^T (rn dz)
//             h16_df_tail        du = [f > 0] rn ([a | dz] [dvlad^T ; Wc^T] - f t_row), sum du, sum du zhat
//             h16_bn_bwd_apply   dz5 = gamma rstd (du - sum du / rows - zhat sum du zhat / rows)    (in place)
//             hx_rowgemm<8>      dcat = dz5 W5^T
//             h16_dw5            dW5 = cat^T dz5
// (hx_*: the templates of train_head_common.h, shared with the f32 head of train_head32.hip)
#include "train_head_common.h"

// ----------------------------------------------------------------------------------------------------------------
// conv5's forward: z5 = bf16(A W5 + b5) with A = cat (rows, 256), f32 or bf16, and the batch statistics of the product.
// A wave's 32 rows are RESIDENT as bf16 fragments (64 registers, read once); W5 streams through double-buffered 16-KB LDS stages (64
// output columns x 128 k) shared by the workgroup's four waves -- global -> LDS by LDS-DMA under the previous stage's products (round 6;
// until then through 16 staging registers and ds_writes: 86.5 -> 82 us at 18 clouds, and with the B fragments read two k-steps ahead of
// their products 80; 93.5 -> 84.6 at 22) -- one
// barrier per stage; a column chunk's result leaves as one dword (two adjacent columns) per lane and row: whole 128-byte runs.  Per stage and wave the
// pivot-shifted column sums go to LDS; 64 threads merge the four waves of the PREVIOUS stage behind the barrier that exists anyway.
// rows a multiple of 32.  stats: [workgroups][3][1024] (tile_rows = 128 for epc_moments_finalize_launch).
// (Round 6, VERDICT r5 #4: SIXTY-FOUR rows per wave -- two A fragments per B-fragment read, 256-row workgroups, 238 registers, two
// workgroups per CU -- was built, was parity-green and measured 103.9 us against 86.5 at 18 clouds (104.7 / 93.9 at 22), pack and
// finalize launches included: half the LDS reads do not pay for a third less occupancy.  Not kept; the other kernels were not rebuilt.)
// ----------------------------------------------------------------------------------------------------------------
#define C5_KS 16
#define C5_STAGE_U4 (8 * 2 * 64)   // 16 KB: half the k-steps of a 64-column chunk ([k-step 8][nt 2][lane])

// Sixteen products of a half-stage: B fragments [k-step 8][nt 2][lane] from LDS, read `AHEAD` k-steps ahead of the products that use them
// (the compiler's own schedule reads a k-step's two fragments, waits, multiplies: an LDS round trip per two MFMAs inside a wave)
template <int AHEAD, int S>
__device__ __forceinline__ void c5_step(const u32x4* __restrict__ B, int lane, const bf16x8* a, u32x4 (&f)[AHEAD + 1][2], f32x16& acc0,
                                        f32x16& acc1) {
    if constexpr (S < 8) {
        if constexpr (S + AHEAD < 8) {
            f[(S + AHEAD) % (AHEAD + 1)][0] = B[((S + AHEAD) * 2 + 0) * 64 + lane];
            f[(S + AHEAD) % (AHEAD + 1)][1] = B[((S + AHEAD) * 2 + 1) * 64 + lane];
        }
        acc0 = mfma_bf16(a[S], __builtin_bit_cast(bf16x8, f[S % (AHEAD + 1)][0]), acc0);
        acc1 = mfma_bf16(a[S], __builtin_bit_cast(bf16x8, f[S % (AHEAD + 1)][1]), acc1);
        if constexpr (S + AHEAD < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // this step's two LDS reads (for k-step S + AHEAD)
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                  // then its two MFMAs
        c5_step<AHEAD, S + 1>(B, lane, a, f, acc0, acc1);
    }
}
template <int AHEAD>
__device__ __forceinline__ void c5_half(const u32x4* __restrict__ B, int lane, const bf16x8* a, f32x16& acc0, f32x16& acc1) {
    u32x4 f[AHEAD + 1][2];
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) f[s][0] = B[(s * 2 + 0) * 64 + lane], f[s][1] = B[(s * 2 + 1) * 64 + lane];
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * AHEAD, 0);
    c5_step<AHEAD, 0>(B, lane, a, f, acc0, acc1);
}

template <bool AF32>
__global__ __launch_bounds__(256, AF32 ? 2 : 3) void h16_conv5_fwd_kernel(const void* __restrict__ A_, int rows, const u32x4* __restrict__ Bp,
                                                                          const float* __restrict__ bias, unsigned* __restrict__ Z,
                                                                          float* __restrict__ stats) {
    // A stage = one HALF (128 k) of a 64-column chunk: 2 x 16 KB of LDS instead of 2 x 32, so that three workgroups share a CU (with the
    // bf16 operand: 144 registers; 42 KB of LDS) and the 576 workgroups of the training tuple are resident at once -- with two per CU the
    // last 64 ran alone in a second round.
    __shared__ u32x4 Bs[2][C5_STAGE_U4];
    __shared__ float wst[2][4][3][64];
    __shared__ bool wlive[4];
    __shared__ float bias_s[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * 128 + wave * 32;
    const bool live = r0 < rows;
    if (lane == 0) wlive[wave] = live;
    constexpr int PER = C5_STAGE_U4 / 256;
    // W5's stages travel global -> LDS by LDS-DMA (no staging registers, no ds_write): a wave moves four 1-KB pieces of a stage.  The
    // target buffer is free when the request is issued (its last readers passed the previous barrier); a wave waits for ITS pieces with a
    // counted s_waitcnt before the barrier that publishes the buffer (vmcnt retires in order: `younger` = the wave's memory operations
    // issued after the request that may still be in flight -- the chunk's sixteen z5 stores).
    const unsigned bs_base = (unsigned)(size_t)(const __attribute__((address_space(3))) u32x4*)&Bs[0][0];
    auto request = [&](int step, int buf) {   // step = 2 chunk + half: the pack is [chunk][k-step][nt][lane], so halves are contiguous
        const float* src = reinterpret_cast<const float*>(Bp + (size_t)step * C5_STAGE_U4);
#pragma unroll
        for (int u = 0; u < PER; ++u)
            glds16(src, 16u * (u * 256 + wave * 64 + lane), bs_base + 16u * (buf * C5_STAGE_U4 + u * 256 + wave * 64));
    };
    request(0, 0);
    bf16x8 ah[C5_KS];
    {
        const size_t row = (size_t)min(r0 + i, rows - 1);
        if constexpr (AF32) {
            const float* p = reinterpret_cast<const float*>(A_) + row * 256 + 8 * h;
#pragma unroll
            for (int s = 0; s < C5_KS; ++s) {
                const float4 x = ld4(p + 16 * s), y = ld4(p + 16 * s + 4);
                const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
                ah[s] = cvt8(v);
            }
        } else {
            const u16* p = reinterpret_cast<const u16*>(A_) + row * 256 + 8 * h;
#pragma unroll
            for (int s = 0; s < C5_KS; ++s) ah[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p + 16 * s));
        }
    }
    // the loop below holds no load the compiler can see (the bias comes from LDS), and its counted waits are ours: the resident fragments
    // are pinned as COMPLETE here -- the compiler's counters do not see the asm waits, and without this it guards every first use of a
    // fragment in every iteration with a counted vmcnt that drains the stage in flight
    for (int e = tid; e < 1024; e += 256) bias_s[e] = bias[e];
#pragma unroll
    for (int s = 0; s < C5_KS; ++s) asm volatile("" : "+v"(ah[s]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const size_t zbase = (size_t)r0 * 512;            // dwords: a row is 512 of them
    const unsigned voff = 4u * h * 512u + i;
    auto flush_stats = [&](int st, int buf) {          // the four waves' sums of chunk st -> one (S1, S2, pivot) per column
        if (tid < 64) {
            float S1, S2, P;
            h16_merge_stats(wst[buf], wlive, tid, S1, S2, P);
            float* o = stats + (size_t)blockIdx.x * 3 * 1024 + 64 * st + tid;
            o[0] = S1, o[1024] = S2, o[2048] = P;
        }
    };
    for (int st = 0; st < 16; ++st) {
        const int sb = st & 1;                         // parity of the statistics buffer
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
        // first half: k-steps 0..7 from buffer 0 (the second half's fragments travel meanwhile)
        if (st > 0) flush_stats(st - 1, sb ^ 1);
        request(2 * st + 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (live) {
            c5_half<2>(Bs[0], lane, ah, acc0, acc1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (nothing younger than the request in this half)
        __syncthreads();
        // second half: k-steps 8..15 from buffer 1, then the chunk's epilogue
        if (st + 1 < 16) request(2 * st + 2, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (live) {
            c5_half<2>(Bs[1], lane, ah + 8, acc0, acc1);
            // D: lane (i, h), register r = row mfma_row(r, h), columns 64 st + 2 i (acc0) and + 1 (acc1).  Pivot = the wave's row 0
            const float p0 = __shfl(acc0[0], i), p1 = __shfl(acc1[0], i);
            float a1 = 0.f, a2 = 0.f, b1s = 0.f, b2s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d0 = acc0[r] - p0, d1 = acc1[r] - p1;
                a1 += d0, a2 += d0 * d0, b1s += d1, b2s += d1 * d1;
            }
            a1 += __shfl_xor(a1, 32), a2 += __shfl_xor(a2, 32), b1s += __shfl_xor(b1s, 32), b2s += __shfl_xor(b2s, 32);
            if (h == 0) {
                wst[sb][wave][0][2 * i] = a1, wst[sb][wave][1][2 * i] = a2, wst[sb][wave][2][2 * i] = p0;
                wst[sb][wave][0][2 * i + 1] = b1s, wst[sb][wave][1][2 * i + 1] = b2s, wst[sb][wave][2][2 * i + 1] = p1;
            }
            const float2 bv = *reinterpret_cast<const float2*>(bias_s + 64 * st + 2 * i);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                unsigned* ob = Z + zbase + (size_t)((r & 3) + 8 * (r >> 2)) * 512 + 32 * st;
                ob[voff] = pack2bf(acc0[r] + bv.x, acc1[r] + bv.y);
            }
        }
        if (live) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");   // (the sixteen z5 stores of this chunk may still travel)
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush_stats(15, 1);
}

// ----------------------------------------------------------------------------------------------------------------
// The VLAD feature gradient continued through conv5's tail backward (train_head.hip's vlad_df_kernel<1, true> on 16-bit tensors):
//     df = [a | dz] [dvlad[b]^T ; Wc^T]  (K = 128);  u = relu(z5 s + t);  f = u rn;  du = [f > 0] (rn df - (rn t_row) f)
// with z5 read and du written as bf16 -- two adjacent columns per lane, so both move as dwords in 128-byte runs (the pack gives the
// two accumulators of a lane adjacent columns).  Column sums (sum du, sum du zhat) from the f32 values, one partial per workgroup.
// ----------------------------------------------------------------------------------------------------------------
#define DF_STAGE_U4 (8 * 2 * 64)   // 16 KB: [k-step 8][nt 2][lane]

// Bp[b][chunk c < 16][s < 8][nt][lane (i, h)][8]: B[k = 16 s + 8 h + j][f = 64 c + 2 i + nt], B = [dvlad[b]^T ; Wc^T]
__global__ __launch_bounds__(256) void h16_df_pack_kernel(const float* __restrict__ dvlad, const float* __restrict__ Wc,
                                                          u32x4* __restrict__ Bp) {
    const int c = blockIdx.x, b = blockIdx.y;
    for (int e = threadIdx.x; e < DF_STAGE_U4; e += 256) {
        const int l = e & 63, nt = (e >> 6) & 1, s = e >> 7, i = l & 31, h = l >> 5;
        const int f = 64 * c + 2 * i + nt, k0 = 16 * s + 8 * h;
        const float* src = k0 < 64 ? dvlad + ((size_t)b * 1024 + f) * 64 + k0 : Wc + (size_t)f * 64 + (k0 - 64);
        const float4 x = ld4(src), y = ld4(src + 4);
        const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        Bp[((size_t)b * 16 + c) * DF_STAGE_U4 + e] = __builtin_bit_cast(u32x4, cvt8(v));
    }
}

struct H16Tail {
    const unsigned* z5;   // (rows, 512) dwords
    const float *rn, *trow;
    H16Bn bn;
    float* partials;      // [workgroups][2][1024]
};

__global__ __launch_bounds__(256, 3) void h16_df_tail_kernel(const float* __restrict__ a, const float* __restrict__ dz,
                                                             const u32x4* __restrict__ Bp, int n_points, unsigned* __restrict__ du,
                                                             H16Tail tail) {
    __shared__ u32x4 Bs[2][DF_STAGE_U4];
    __shared__ __attribute__((aligned(16))) float coef[4][1024];   // s, t, mean, rstd
    __shared__ float rowc[4][2][32];
    __shared__ float psum[2][4][2][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int r0 = (blockIdx.x * 4 + wave) * 32;
    const bool live = r0 < n_points;
    const size_t row = (size_t)b * n_points + min(r0 + i, n_points - 1);
    const u32x4* src = Bp + (size_t)b * 16 * DF_STAGE_U4;
    // the operand's stages travel global -> LDS by LDS-DMA, a wave four 1-KB pieces of a stage (h16_conv5_fwd_kernel's scheme: the counted
    // wait in front of the barrier leaves the wave's younger operations -- the next z5 values, this stage's du stores -- in flight)
    constexpr int PER = DF_STAGE_U4 / 256;
    const unsigned bs_base = (unsigned)(size_t)(const __attribute__((address_space(3))) u32x4*)&Bs[0][0];
    auto request = [&](int st, int buf) {
        const float* from = reinterpret_cast<const float*>(src + (size_t)st * DF_STAGE_U4);
#pragma unroll
        for (int u = 0; u < PER; ++u)
            glds16(from, 16u * (u * 256 + wave * 64 + lane), bs_base + 16u * (buf * DF_STAGE_U4 + u * 256 + wave * 64));
    };
    request(0, 0);
    bf16x8 ah[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const float* p = (s < 4 ? a : dz) + row * 64 + 16 * (s & 3) + 8 * h;
        const float4 x = ld4(p), y = ld4(p + 4);
        const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        ah[s] = cvt8(v);
    }
    for (int c = tid; c < 1024; c += 256) {
        const float rs = 1.0f / sqrtf(tail.bn.var[c] + tail.bn.eps);
        const BnAffine af = bn_affine(tail.bn.mean[c], tail.bn.var[c], tail.bn.gamma[c], tail.bn.beta[c], tail.bn.eps);
        coef[0][c] = af.s, coef[1][c] = af.t, coef[2][c] = tail.bn.mean[c], coef[3][c] = rs;
    }
    if (h == 0) {
        const float rnv = live ? tail.rn[row] : 0.f, tv = live ? tail.trow[row] : 0.f;
        rowc[wave][0][i] = rnv;
        rowc[wave][1][i] = rnv >= 0.99e6f ? 0.f : rnv * tv;
    }
    // (the resident fragments pinned as complete: the compiler's counters do not see the asm waits of the loop -- h16_conv5_fwd_kernel)
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(ah[s]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    const size_t tile_base = ((size_t)b * n_points + r0) * 512;   // dwords
    const unsigned voff = 4u * h * 512u + i;
    unsigned zn[16];
    auto zload = [&](int st) {
#pragma unroll
        for (int r = 0; r < 16; ++r) zn[r] = (tail.z5 + tile_base + (size_t)((r & 3) + 8 * (r >> 2)) * 512 + 32 * st)[voff];
    };
    if (live) zload(0);
    auto flush = [&](int st, int buf) {      // stage st's column sums: four waves -> one partial
        if (tid < 128) {
            const int q = tid >> 6, c = tid & 63;
            const float v = (psum[buf][0][q][c] + psum[buf][1][q][c]) + (psum[buf][2][q][c] + psum[buf][3][q][c]);
            tail.partials[((size_t)wg * 2 + q) * 1024 + 64 * st + c] = v;
        }
    };
    for (int st = 0; st < 16; ++st) {
        const int buf = st & 1;
        unsigned zv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) zv[r] = zn[r];
        if (st + 1 < 16) request(st + 1, buf ^ 1);      // (the buffer's last readers passed the barrier at the end of the previous stage)
        if (live && st + 1 < 16) zload(st + 1);
        if (st > 0) flush(st - 1, buf ^ 1);
        __builtin_amdgcn_sched_barrier(0);
        if (live) {
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
            c5_half<2>(Bs[buf], lane, ah, acc0, acc1);
            const int c0 = 64 * st + 2 * i;
            const float2 cs = *reinterpret_cast<const float2*>(&coef[0][c0]), ct = *reinterpret_cast<const float2*>(&coef[1][c0]);
            const float2 mu = *reinterpret_cast<const float2*>(&coef[2][c0]), rs = *reinterpret_cast<const float2*>(&coef[3][c0]);
            float s10 = 0.f, s20 = 0.f, s11 = 0.f, s21 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = mfma_row(r, h);
                const float rnv = rowc[wave][0][rr], rt = rowc[wave][1][rr];
                const float z0 = bf_lo(zv[r]), z1 = bf_hi(zv[r]);
                const float f0 = fmaxf(z0 * cs.x + ct.x, 0.f) * rnv, f1 = fmaxf(z1 * cs.y + ct.y, 0.f) * rnv;
                const float d0 = f0 > 0.f ? rnv * acc0[r] - rt * f0 : 0.f;
                const float d1 = f1 > 0.f ? rnv * acc1[r] - rt * f1 : 0.f;
                s10 += d0, s20 += d0 * ((z0 - mu.x) * rs.x);
                s11 += d1, s21 += d1 * ((z1 - mu.y) * rs.y);
                (du + tile_base + (size_t)((r & 3) + 8 * (r >> 2)) * 512 + 32 * st)[voff] = pack2bf(d0, d1);
            }
            s10 += __shfl_xor(s10, 32), s20 += __shfl_xor(s20, 32), s11 += __shfl_xor(s11, 32), s21 += __shfl_xor(s21, 32);
            if (h == 0) {
                psum[buf][wave][0][2 * i] = s10, psum[buf][wave][1][2 * i] = s20;
                psum[buf][wave][0][2 * i + 1] = s11, psum[buf][wave][1][2 * i + 1] = s21;
            }
        } else if (h == 0) {
            psum[buf][wave][0][2 * i] = 0.f, psum[buf][wave][1][2 * i] = 0.f;
            psum[buf][wave][0][2 * i + 1] = 0.f, psum[buf][wave][1][2 * i + 1] = 0.f;
        }
        // younger than the request: the sixteen z5 loads of the next stage (when there is one) and this stage's sixteen du stores (+ one
        // partial's store on two of the waves)
        if (live && st + 1 < 16) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
        else if (live) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    flush(15, 1);
}

// ----------------------------------------------------------------------------------------------------------------
// dz5 = gamma rstd (du - sum du / rows - zhat sum du zhat / rows) on bf16 rows, in place or not: the last step of conv5's BatchNorm
// backward (utils/tf_util.py:454-519 from the gradient side) once the column sums are known.  A wave takes whole 2-KB rows, 16 bytes
// per lane and half row; the sixteen channels of a lane keep their coefficients in registers.
// ----------------------------------------------------------------------------------------------------------------
#define BA_ROWS 16   // rows per workgroup (4 per wave)

__global__ __launch_bounds__(256) void h16_bn_bwd_apply_kernel(const u32x4* __restrict__ du, const u32x4* __restrict__ z5, H16Bn bn,
                                                               const float* __restrict__ dbeta, const float* __restrict__ dgamma,
                                                               float inv_rows, int rows, u32x4* __restrict__ dz) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mu[16], k1[16], bb[16], gg[16];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 512 * u + 8 * lane + e, k = 8 * u + e;
            const float r = 1.0f / sqrtf(bn.var[c] + bn.eps);
            mu[k] = bn.mean[c], k1[k] = bn.gamma[c] * r, bb[k] = dbeta[c] * inv_rows, gg[k] = r * (dgamma[c] * inv_rows);
        }
    const int row0 = blockIdx.x * BA_ROWS + wave;
#pragma unroll
    for (int q = 0; q < BA_ROWS / 4; ++q) {
        const int row = row0 + 4 * q;
        if (row >= rows) break;
        const size_t o = (size_t)row * 128 + lane;     // u32x4 units: a row is 128 of them
        const u32x4 g0 = du[o], g1 = du[o + 64], z0 = z5[o], z1 = z5[o + 64];
        u32x4 o0, o1;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float a = k1[2 * w] * (bf_lo(g0[w]) - bb[2 * w] - (bf_lo(z0[w]) - mu[2 * w]) * gg[2 * w]);
            const float b = k1[2 * w + 1] * (bf_hi(g0[w]) - bb[2 * w + 1] - (bf_hi(z0[w]) - mu[2 * w + 1]) * gg[2 * w + 1]);
            o0[w] = pack2bf(a, b);
            const float c = k1[8 + 2 * w] * (bf_lo(g1[w]) - bb[8 + 2 * w] - (bf_lo(z1[w]) - mu[8 + 2 * w]) * gg[8 + 2 * w]);
            const float d = k1[9 + 2 * w] * (bf_hi(g1[w]) - bb[9 + 2 * w] - (bf_hi(z1[w]) - mu[9 + 2 * w]) * gg[9 + 2 * w]);
            o1[w] = pack2bf(c, d);
        }
        dz[o] = o0, dz[o + 64] = o1;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// conv5's weight gradient dW5 (256, 1024) = cat^T dz5 -- both operands (rows, .) row-major with the ROWS as the contraction, 73 728 deep at
// the training tuple's size; the MFMA wants 8 consecutive rows of ONE channel per lane.  The generic tile GEMM took 163 us for it (2-byte
// lane-coalesced fetches, operands re-split per tile); a first kernel here that fetched 8 / 4 bytes per lane straight into fragments and
// re-read cat once per 128-column tile took 171 us, with 256-column tiles 97 us: hundreds of narrow load instructions per step and CU.
// This one moves every byte ONCE per workgroup, 16 bytes per lane:
//   * a workgroup (8 waves) owns all 256 input channels x 256 output columns over a slice of the rows, 64 rows per step;
//   * wave w < 4 loads rows 16 w .. + 15 of cat (lane = 8 channels x 8 rows: eight 16-byte loads, two whole 512-byte rows per
//     instruction), waves 4 .. 7 the same of dz5's 256 columns; an 8 x 8 transposition of 16-bit values in registers (32 byte-permutes)
//     turns a lane's 8 rows x 8 channels into 8 fragment entries (8 rows of one channel each), written to LDS in fragment order;
//   * after ONE barrier per step wave (wm, wn) reads its 4 + 2 fragments per k-step (conflict-free 16-byte reads) for a 128 x 64 tile:
//     32 MFMAs per step and wave; LDS is double-buffered (2 x 64 KB), the next step's rows travel under the products.
// Slices are added in ascending order by h16_partial_reduce_kernel (no atomics: the same bits every run).
// (Round 6: putting the four column tiles of a row slice on ONE XCD -- workgroups go to the XCDs round-robin by linear id, the four read
// the same cat rows -- measured 83.5 / 101.9 us against 86.0 / 85.9 at 18 clouds and 121 against 109 at 22: not kept.)
// ----------------------------------------------------------------------------------------------------------------
#define DW_STEP_U4 (4 * 8 * 64)   // one operand of one 64-row step: [k-step 4][tile 8][lane 64] x 16 bytes = 32 KB

// 8 rows x 8 sixteen-bit values (in[j] = the 8 values of row j) -> out[q] = the 8 rows of value q
__device__ __forceinline__ void h16_transpose8x8(const u32x4 (&in)[8], u32x4 (&out)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int d = 0; d < 4; ++d)
            out[q][d] = __builtin_amdgcn_perm(in[2 * d + 1][q >> 1], in[2 * d][q >> 1], (q & 1) ? 0x07060302u : 0x05040100u);
}

template <bool AF32>
__global__ __launch_bounds__(512, 1) void h16_dw5_kernel(const void* __restrict__ cat_, const u16* __restrict__ dz5, int rows,
                                                         int rows_per_wg, float* __restrict__ P) {
    extern __shared__ u32x4 dw_lds[];                  // [buffer 2][operand 2][DW_STEP_U4]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int n0 = blockIdx.x * 256;
    const int rbeg = blockIdx.y * rows_per_wg, rend = min(rbeg + rows_per_wg, rows);
    // loader role: operand (0 = cat, 1 = dz5), rows 16 piece + 8 hh + j of the step, values 8 c .. 8 c + 7
    const int oper = wave >> 2, piece = wave & 3, c = lane & 31, hh = lane >> 5;
    const int last = max(rend - 1, rbeg);
    u32x4 in[8];
    // Every load of a step is UNCONDITIONAL and the rows past the slice are zeroed at deposit time: a load guarded per lane (the first form of
    // this lambda: `if (row >= rend) in[j] = 0` right behind it) is compiled into load, s_waitcnt vmcnt(0), select -- eight dependent round
    // trips per step instead of eight loads in flight (found in the ISA in round 6).
    auto load = [&](int rb) {
        const int r0 = rb + 16 * piece + 8 * hh;
        if (oper == 0) {
            if constexpr (AF32) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float* p = reinterpret_cast<const float*>(cat_) + (size_t)min(r0 + j, last) * 256 + 8 * c;
                    const float4 x = ld4(p), y = ld4(p + 4);
                    const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
                    in[j] = __builtin_bit_cast(u32x4, cvt8(v));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    in[j] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const u16*>(cat_) + (size_t)min(r0 + j, last) * 256 + 8 * c);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) in[j] = *reinterpret_cast<const u32x4*>(dz5 + (size_t)min(r0 + j, last) * 1024 + n0 + 8 * c);
        }
    };
    // fragment entry of value q of this lane: k-step = piece, tile = c >> 2, lane (i = 8 (c & 3) + q, h = hh).  Entry L of tile T sits at
    // position L ^ T of the tile's 64: one write instruction (fixed q) then spreads its 64 lanes over all 16-byte bank groups -- in
    // lane order every lane of it landed on two of the sixteen (a 32-way conflict: the first version of this kernel took 99 us)
    const int wr_tile = c >> 2;
    const int wr_base = oper * DW_STEP_U4 + (piece * 8 + wr_tile) * 64;
    const int wr_lane = 32 * hh + 8 * (c & 3);
    auto deposit = [&](int buf, int rb) {         // rb: the step whose rows `in` holds
        if (oper == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (rb + 16 * piece + 8 * hh + j >= rend) in[j] = u32x4{0u, 0u, 0u, 0u};   // (a row past the slice contributes zeros)
        }
        u32x4 out[8];
        h16_transpose8x8(in, out);
#pragma unroll
        for (int q = 0; q < 8; ++q) dw_lds[buf * 2 * DW_STEP_U4 + wr_base + ((wr_lane + q) ^ wr_tile)] = out[q];
    };
    f32x16 acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][t][r] = 0.f;
    if (rbeg < rend) {
        load(rbeg);
        deposit(0, rbeg);
    }
    __syncthreads();
    int buf = 0;
    for (int rb = rbeg; rb < rend; rb += 64, buf ^= 1) {
        const bool more = rb + 64 < rend;
        if (more) load(rb + 64);
        __builtin_amdgcn_sched_barrier(0);
        const u32x4* As = dw_lds + buf * 2 * DW_STEP_U4;
        const u32x4* Bs = As + DW_STEP_U4;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 a[4], b[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = __builtin_bit_cast(bf16x8, As[(ks * 8 + 4 * wm + q) * 64 + (lane ^ (4 * wm + q))]);
#pragma unroll
            for (int t = 0; t < 2; ++t) b[t] = __builtin_bit_cast(bf16x8, Bs[(ks * 8 + 2 * wn + t) * 64 + (lane ^ (2 * wn + t))]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[q][t] = mfma_bf16(a[q], b[t], acc[q][t]);
        }
        if (more) deposit(buf ^ 1, rb + 64);    // (the other buffer: its last readers passed the barrier at the end of the previous step)
        __syncthreads();
    }
    // D: lane (i, h), register r of (q, t) = dW5[channel 128 wm + 32 q + mfma_row(r, h)][column n0 + 64 wn + 32 t + i]
    const int i = lane & 31, h = lane >> 5;
    float* o = P + (size_t)blockIdx.y * 256 * 1024 + n0 + 64 * wn + i;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 128 * wm + 32 * q + mfma_row(r, h);
#pragma unroll
            for (int t = 0; t < 2; ++t) o[(size_t)ch * 1024 + 32 * t] = acc[q][t][r];
        }
}

// bf16 rows -> f32 (test taps, the materialised features of the distillation variants): y = T(z) with T = identity, or
// relu(batch_norm(z)) rn (the feature map f the fused kernels never write)
__global__ __launch_bounds__(256) void h16_expand_kernel(const unsigned* __restrict__ z, H16Bn bn, const float* __restrict__ rn,
                                                         long n_dwords, float* __restrict__ y) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_dwords) return;
    const unsigned w = z[e];
    float a = bf_lo(w), b = bf_hi(w);
    if (bn.mean) {
        const int c = (int)((2 * e) & 1023);
        const BnAffine a0 = bn_affine(bn.mean[c], bn.var[c], bn.gamma[c], bn.beta[c], bn.eps);
        const BnAffine a1 = bn_affine(bn.mean[c + 1], bn.var[c + 1], bn.gamma[c + 1], bn.beta[c + 1], bn.eps);
        const float r = rn ? rn[(2 * e) >> 10] : 1.f;
        a = fmaxf(a * a0.s + a0.t, 0.f) * r, b = fmaxf(b * a1.s + a1.t, 0.f) * r;
    }
    *reinterpret_cast<float2*>(y + 2 * e) = make_float2(a, b);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------

// conv5's scratch: W5 packed (256 x 1024 bf16) | the moments' partials, 3 x 1024 per 128-row workgroup (wgs of them)
struct h16_conv5_ws { int wgs; u32x4* pack; float* stats; size_t bytes; };
static h16_conv5_ws h16_conv5_layout(void* base, int rows) {
    epc_carver c(base);
    const int wgs = (rows + 127) / 128;
    return {wgs, c.take<u32x4>(256 * 1024 * 2 / sizeof(u32x4)), c.take<float>((size_t)wgs * 3 * 1024), c.bytes()};
}

extern "C" size_t epc_h16_conv5_fwd_scratch_bytes(int rows) { return rows > 0 ? h16_conv5_layout(nullptr, rows).bytes : 0; }

extern "C" int epc_h16_conv5_fwd(const void* cat, int cat_is_bf16, const float* W5, const float* b5, int rows, void* z5, float* mean,
                                 float* var, void* scratch, size_t scratch_bytes, void* stream) {
    EPC_CHECK_ARG(cat && W5 && b5 && z5 && mean && var && scratch, "null pointer");
    EPC_CHECK_ARG(rows > 0 && rows % 32 == 0 && (long)rows * 1024 < (1L << 32), "rows must be a positive multiple of 32 (rows * 1024 < 2^32)");
    EPC_CHECK_ARG(scratch_bytes >= epc_h16_conv5_fwd_scratch_bytes(rows), "scratch too small (epc_h16_conv5_fwd_scratch_bytes)");
    EPC_CHECK_ARG(epc_aligned16(cat) && epc_aligned16(z5) && epc_aligned16(scratch) && epc_aligned16(b5), "tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const h16_conv5_ws w = h16_conv5_layout(scratch, rows);
    h16_pack<1>(W5, 1024, 1, 0, 1, 256, 1024, 0, 4, w.pack, st);
    if (cat_is_bf16)
        hipLaunchKernelGGL(h16_conv5_fwd_kernel<false>, dim3(w.wgs), dim3(256), 0, st, cat, rows, (const u32x4*)w.pack, b5, (unsigned*)z5, w.stats);
    else
        hipLaunchKernelGGL(h16_conv5_fwd_kernel<true>, dim3(w.wgs), dim3(256), 0, st, cat, rows, (const u32x4*)w.pack, b5, (unsigned*)z5, w.stats);
    epc_moments_finalize_launch(w.stats, w.wgs, 1024, rows, 128, b5, mean, var, stream);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

// The entry points shared with train_head32.hip (train_head_common.h has their bodies): bf16 rows, one bf16 piece per operand
struct H16Arith {
    typedef u16 T;
    static constexpr const char* NAME = "epc_h16";
    static constexpr int P = 1, KSC_ASSIGN = 4, KSC_DX = 4, ASSIGN_SLOTS = 4, COL_TILES = 8, ASSIGN_PACK_BYTES = 2;
};

extern "C" size_t epc_h16_assign_scratch_bytes(int num_clouds, int n_points, int per_cloud_operand) {
    return hx_assign_scratch_bytes<H16Arith>(num_clouds, n_points, per_cloud_operand);
}
extern "C" int epc_h16_assign(const void* z5, const float* mean5, const float* var5, const float* gamma5, const float* beta5, float eps,
                              const float* B, int per_cloud_operand, int num_clouds, int n_points, float* out, float* rn_out,
                              float* mean_out, float* var_out, void* scratch, size_t scratch_bytes, void* stream) {
    return hx_assign<H16Arith>((const u16*)z5, mean5, var5, gamma5, beta5, eps, B, per_cloud_operand, num_clouds, n_points, out, rn_out, mean_out,
                               var_out, scratch, scratch_bytes, stream);
}

extern "C" size_t epc_h16_dx_scratch_bytes(void) { return hx_dx_scratch_bytes<H16Arith>(); }
extern "C" int epc_h16_conv5_dx(const void* dz5, const float* W5, int rows, float* dcat, void* scratch, size_t scratch_bytes, void* stream) {
    return hx_conv5_dx<H16Arith>((const u16*)dz5, W5, rows, dcat, scratch, scratch_bytes, stream);
}
// (epc_h16_bn_bwd_apply and epc_h16_conv5_dx in one pass; dz5 may be du)
extern "C" int epc_h16_conv5_dx_bn(const void* du, const void* z5, const float* mean5, const float* var5, const float* gamma5, float eps,
                                   const float* dbeta, const float* dgamma, const float* W5, int rows, void* dz5, float* dcat, void* scratch,
                                   size_t scratch_bytes, void* stream) {
    return hx_conv5_dx_bn<H16Arith>((const u16*)du, (const u16*)z5, mean5, var5, gamma5, eps, dbeta, dgamma, W5, rows, (u16*)dz5, dcat, scratch,
                                    scratch_bytes, stream);
}

extern "C" size_t epc_h16_colgemm_scratch_bytes(int num_clouds, int n_points) { return hx_colgemm_scratch_bytes<H16Arith>(num_clouds, n_points); }
extern "C" int epc_h16_colgemm(const void* z5, const float* mean5, const float* var5, const float* gamma5, const float* beta5, float eps,
                               const float* C, const float* rn, int num_clouds, int n_points, int per_cloud, float* out, void* scratch,
                               size_t scratch_bytes, void* stream) {
    return hx_colgemm<H16Arith>((const u16*)z5, mean5, var5, gamma5, beta5, eps, C, rn, num_clouds, n_points, per_cloud, out, scratch, scratch_bytes,
                                stream);
}

// the tail's scratch: dvlad Wc^T packed (16 stages per cloud) | (sum du, sum du zhat) partials, 2 x 1024 per 128-row workgroup (`tiles` per cloud)
struct h16_df_ws { int tiles; u32x4* pack; float* partials; size_t bytes; };
static h16_df_ws h16_df_layout(void* base, int num_clouds, int n_points) {
    epc_carver c(base);
    const int tiles = (n_points + 127) / 128;
    return {tiles, c.take<u32x4>((size_t)num_clouds * 16 * DF_STAGE_U4), c.take<float>((size_t)num_clouds * tiles * 2 * 1024), c.bytes()};
}

extern "C" size_t epc_h16_df_tail_scratch_bytes(int num_clouds, int n_points) {
    return num_clouds > 0 && n_points > 0 ? h16_df_layout(nullptr, num_clouds, n_points).bytes : 0;
}

// du (rows, 1024) bf16 and dbeta_dgamma (2, 1024) = (sum du, sum du zhat): see h16_df_tail_kernel
extern "C" int epc_h16_df_tail(const float* a, const float* dz, const float* dvlad, const float* Wc, int num_clouds, int n_points,
                               const void* z5, const float* rn, const float* trow, const float* mean5, const float* var5,
                               const float* gamma5, const float* beta5, float eps, void* du, float* dbeta_dgamma, void* scratch,
                               size_t scratch_bytes, void* stream) {
    EPC_CHECK_ARG(a && dz && dvlad && Wc && z5 && rn && trow && mean5 && var5 && gamma5 && beta5 && du && dbeta_dgamma && scratch, "null pointer");
    EPC_CHECK_ARG(num_clouds > 0 && num_clouds <= 65535 && n_points > 0 && n_points % 32 == 0 && (long)num_clouds * n_points * 1024 < (1L << 32),
                  "bad shape (n_points a multiple of 32; rows * 1024 < 2^32)");
    EPC_CHECK_ARG(scratch_bytes >= epc_h16_df_tail_scratch_bytes(num_clouds, n_points), "scratch too small (epc_h16_df_tail_scratch_bytes)");
    EPC_CHECK_ARG(epc_aligned16(a) && epc_aligned16(dz) && epc_aligned16(dvlad) && epc_aligned16(Wc) && epc_aligned16(z5) && epc_aligned16(du) &&
                      epc_aligned16(scratch) && epc_aligned16(dbeta_dgamma),
                  "tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const h16_df_ws w = h16_df_layout(scratch, num_clouds, n_points);
    hipLaunchKernelGGL(h16_df_pack_kernel, dim3(16, num_clouds), dim3(256), 0, st, dvlad, Wc, w.pack);
    const H16Tail tail{(const unsigned*)z5, rn, trow, H16Bn{mean5, var5, gamma5, beta5, eps}, w.partials};
    hipLaunchKernelGGL(h16_df_tail_kernel, dim3(w.tiles, num_clouds), dim3(256), 0, st, a, dz, (const u32x4*)w.pack, n_points, (unsigned*)du, tail);
    epc_partial_sum_wide_launch(w.partials, w.tiles * num_clouds, 2 * 1024, dbeta_dgamma, stream);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

extern "C" int epc_h16_bn_bwd_apply(const void* du, const void* z5, const float* mean5, const float* var5, const float* gamma5,
                                    const float* beta5, float eps, const float* dbeta, const float* dgamma, int rows, void* dz5,
                                    void* stream) {
    EPC_CHECK_ARG(du && z5 && mean5 && var5 && gamma5 && beta5 && dbeta && dgamma && dz5, "null pointer");
    EPC_CHECK_ARG(rows > 0, "bad shape");
    EPC_CHECK_ARG(epc_aligned16(du) && epc_aligned16(z5) && epc_aligned16(dz5), "tensors must be 16-byte aligned");
    const H16Bn bn{mean5, var5, gamma5, beta5, eps};
    hipLaunchKernelGGL(h16_bn_bwd_apply_kernel, dim3((rows + BA_ROWS - 1) / BA_ROWS), dim3(256), 0, (hipStream_t)stream, (const u32x4*)du,
                       (const u32x4*)z5, bn, dbeta, dgamma, 1.0f / rows, rows, (u32x4*)dz5);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

static int h16_dw5_splits(int rows) { return hx_dw5_splits(rows, 64); }

extern "C" size_t epc_h16_conv5_dw_scratch_bytes(int rows) {
    return rows > 0 ? (size_t)h16_dw5_splits(rows) * 256 * 1024 * sizeof(float) : 0;
}

// dW5 (256, 1024) f32 = cat^T dz5: cat (rows, 256) f32 (or bf16: cat_is_bf16), rounded to bf16 as it is loaded; dz5 (rows, 1024) bf16
extern "C" int epc_h16_conv5_dw(const void* cat, int cat_is_bf16, const void* dz5, int rows, float* dW5, void* scratch, size_t scratch_bytes,
                                void* stream) {
    EPC_CHECK_ARG(cat && dz5 && dW5 && scratch, "null pointer");
    EPC_CHECK_ARG(rows > 0 && (long)rows * 1024 < (1L << 32), "bad shape");
    EPC_CHECK_ARG(scratch_bytes >= epc_h16_conv5_dw_scratch_bytes(rows), "scratch too small (epc_h16_conv5_dw_scratch_bytes)");
    EPC_CHECK_ARG(epc_aligned16(cat) && epc_aligned16(dz5) && epc_aligned16(dW5) && epc_aligned16(scratch), "tensors must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int S = h16_dw5_splits(rows);
    const int rows_per_wg = ((rows + S - 1) / S + 63) / 64 * 64;
    const size_t lds = (size_t)2 * 2 * DW_STEP_U4 * sizeof(u32x4);     // 128 KB
    const void* fn = cat_is_bf16 ? reinterpret_cast<const void*>(h16_dw5_kernel<false>) : reinterpret_cast<const void*>(h16_dw5_kernel<true>);
    EPC_SET_DYN_LDS(fn, lds);
    if (cat_is_bf16)
        hipLaunchKernelGGL(h16_dw5_kernel<false>, dim3(4, S), dim3(512), lds, st, cat, (const u16*)dz5, rows, rows_per_wg, (float*)scratch);
    else
        hipLaunchKernelGGL(h16_dw5_kernel<true>, dim3(4, S), dim3(512), lds, st, cat, (const u16*)dz5, rows, rows_per_wg, (float*)scratch);
    const long per = 256 * 1024;
    hipLaunchKernelGGL(h16_partial_reduce_kernel, dim3((unsigned)(per / 4 / 256), 1), dim3(256), 0, st, (const float*)scratch, S, per, dW5);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

// y (rows, 1024) f32 from bf16 rows: the values themselves (mean5 = NULL), or the feature map relu(bn(z5)) rn (rn may be NULL: no row
// factor) -- what the fused kernels never write; for test taps and the distillation variants' second output.
extern "C" int epc_h16_expand(const void* z, const float* mean5, const float* var5, const float* gamma5, const float* beta5, float eps,
                              const float* rn, int rows, float* y, void* stream) {
    EPC_CHECK_ARG(z && y && rows > 0, "bad argument");
    EPC_CHECK_ARG(!mean5 || (var5 && gamma5 && beta5), "the BatchNorm's four tensors come together");
    const long n = (long)rows * 512;
    const H16Bn bn{mean5, var5, gamma5, beta5, eps};
    hipLaunchKernelGGL(h16_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)z, bn, rn, n, y);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
