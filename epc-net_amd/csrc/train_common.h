// ONE definition of the primitives the training step's three kernel families share -- the per-layer operators (train_ops.hip,
// train_head.hip, train_hidden.hip), the streamed conv5 / VLAD head (train_head_common.h) and the fused backbone chain
// (train_chain_common.h) -- so that kernels under a bit-for-bit contract with each other round alike (as conv1_quad of common.h
// does for the inference path).  (The launchers' host helpers, epc_aligned16 and epc_set_dyn_lds, are in common.h.)
#pragma once
#include "common.h"

// The BatchNorm affine y = z * s + t.  THE CONTRACT: the forward and every ReLU mask the backward recomputes -- per layer, in the
// streamed head and in the fused chain -- evaluate this expression and no other (same association, z * s + t contracted to one FMA),
// so that they agree bit for bit; the tests that compare the fused paths with the per-layer ones element by element depend on it.
struct BnAffine {
    float s, t;
};
__device__ __forceinline__ BnAffine bn_affine(float mean, float var, float gamma, float beta, float eps) {
    BnAffine a;
    a.s = (1.0f / sqrtf(var + eps)) * gamma;
    a.t = beta - mean * a.s;
    return a;
}
__device__ __forceinline__ float bn_value(float z, const BnAffine& a) { return z * a.s + a.t; }

// P bf16 pieces of 8 values: p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1)  (8 significant bits each).  Three named
// pieces (the per-layer operators) or an array of P (pieces a caller does not ask for are dead code).
__device__ __forceinline__ void bf16_split(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        p0[j] = (__bf16)v[j];
        const float r1 = v[j] - (float)p0[j];
        p1[j] = (__bf16)r1;
        p2[j] = (__bf16)(r1 - (float)p1[j]);
    }
}
template <int P>
__device__ __forceinline__ void bf16_split(const float (&v)[8], bf16x8 (&p)[P]) {
    bf16x8 none[2];
    if constexpr (P == 3) bf16_split(v, p[0], p[1], p[2]);
    else if constexpr (P == 2) bf16_split(v, p[0], p[1], none[0]);
    else bf16_split(v, p[0], none[0], none[1]);
}
// acc += a (P pieces) times b (P pieces), the products whose piece indices sum to less than P, smallest terms first: P = 1 one
// product (the bf16 arithmetic), P = 2 three (2^-16 per product: the backward arithmetic of epc_gemm_f32_fast), P = 3 six
// (f32-accurate: epc_gemm_f32's).  The ORDER of the products is part of the result (each MFMA rounds into the accumulator): for
// P = 3 it is a2 b0, a0 b2, a1 b1, a1 b0, a0 b1, a0 b0 -- do not reorder.
template <int P>
__device__ __forceinline__ f32x16 bf16_prod(const bf16x8 (&a)[P], const bf16x8 (&b)[P], f32x16 acc) {
    if constexpr (P == 3) {
        acc = mfma_bf16(a[2], b[0], acc);
        acc = mfma_bf16(a[0], b[2], acc);
        acc = mfma_bf16(a[1], b[1], acc);
    }
    if constexpr (P >= 2) {
        acc = mfma_bf16(a[1], b[0], acc);
        acc = mfma_bf16(a[0], b[1], acc);
    }
    return mfma_bf16(a[0], b[0], acc);
}

// The transposition image: the bf16 pieces of a 32-row x 64-channel tile in LDS as [row][channel] (128-B rows, 16-B chunks
// XOR-swizzled), read back TRANSPOSED by ds_read_b64_tr_b16 -- lane 4q + p of a 16-lane group addresses row r0 + q, channels
// c0 + 4p .. + 3; lane i receives channel c0 + i of the four rows -- for the products that contract over the rows (dW = x^T dz).
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define BF16_IMG_BYTES 4096   // one piece: 32 rows x 128 B
__device__ __forceinline__ int bf16_img_off(int row, int chunk) {   // byte offset of 16-byte chunk `chunk` (0..7) of row `row`
    return 128 * row + 16 * (chunk ^ (((row >> 1) & 1) << 2) ^ (((row >> 2) & 1) << 1));
}
// the A / B fragment (k = rows 16 s2 + 8 h .. + 7, m or n = channel 32 t + (lane & 31)) of one piece, read transposed
__device__ __forceinline__ bf16x8 bf16_tr_frag(const char* img, int t, int s2, int lane) {
    const int g16 = lane >> 4, l16 = lane & 15, q = l16 >> 2, pp = l16 & 3;
    const int chunk = 4 * t + 2 * (g16 & 1) + (pp >> 1);
    const int r0 = 16 * s2 + 8 * (g16 >> 1);
    typedef __attribute__((address_space(3))) s16x4* lds_ptr;
    const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(img + bf16_img_off(r0 + q, chunk) + 8 * (pp & 1)));
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(img + bf16_img_off(r0 + 4 + q, chunk) + 8 * (pp & 1)));
    const s16x8 v = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// The neighbour mean of point `pt` (models/epc-net.py:70-72) for one lane's four channels 4 q .. 4 q + 3 of the (rows, 64) tensor z4:
// (sum over the point's selected neighbours of act(row)) / kdiv.  `act` is what is applied to a row as it is loaded: the identity for
// a tensor that exists (neighbour_mean_kernel), relu(bn0(.)) for the chain's gathers, where x is never written.  THE ORDER of the
// additions is part of the result, and every caller gets this one:
//   * a list of at most `cap` entries (cnt <= cap): when it has 20 or more and cap % 4 == 0, its first 20 entries come as five int4
//     index loads, their 20 rows are in flight at once (the one-at-a-time loop chains 20 dependent (index, row) round trips; every
//     ordinary row has at least 20) and are added in list order; then the tail, one entry at a time, in list order;
//   * more than `cap` selected entries (exact ties: duplicated / zero-padded clouds): the exact scan over the cloud's points j in
//     ascending order with the selection's own test, -|p_i - p_j|^2 >= kth.
// OFF is the offset type of the 20 rows in flight: size_t, or unsigned where the caller knows rows * 16 < 2^32 (the persistent chain).
// (The point's own row, act(z4[pt * 16 + q]) for d = xm - x, is the caller's one line: loaded in here and returned beside the mean it
// cost the persistent chain 8 VGPRs, 153 -> 161 of its 168.)
struct NbIdentity {
    __device__ __forceinline__ float4 operator()(const float4& v) const { return v; }
};
template <typename OFF, typename ACT>
__device__ __forceinline__ float4 neighbour_mean_of(const float4* z4, const float* xyz, const int32_t* idx, const int32_t* cnt,
                                                    const float* kth, int cap, int n, float kdiv, int pt, int q, ACT act) {
    const int cloud_base = (pt / n) * n;
    const int c = cnt[pt];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto add = [&](const float4& v) {
        const float4 y = act(v);
        acc.x += y.x, acc.y += y.y, acc.z += y.z, acc.w += y.w;
    };
    if (c <= cap) {
        int m = 0;
        if (c >= 20 && cap % 4 == 0) {
            const int4* il = reinterpret_cast<const int4*>(idx + (size_t)pt * cap);
            int nb[20];
#pragma unroll
            for (int m4 = 0; m4 < 5; ++m4) {
                const int4 tq = il[m4];
                nb[4 * m4] = tq.x, nb[4 * m4 + 1] = tq.y, nb[4 * m4 + 2] = tq.z, nb[4 * m4 + 3] = tq.w;
            }
            float4 v[20];
#pragma unroll
            for (int u = 0; u < 20; ++u) v[u] = z4[(OFF)(cloud_base + nb[u]) * (OFF)16 + (OFF)q];
#pragma unroll
            for (int u = 0; u < 20; ++u) add(v[u]);
            m = 20;
        }
        for (; m < c; ++m) add(z4[(size_t)(cloud_base + idx[(size_t)pt * cap + m]) * 16 + q]);
    } else {
        const float* pc = xyz + (size_t)cloud_base * 3;
        const int ii = pt - cloud_base;
        const float xi = pc[3 * ii], yi = pc[3 * ii + 1], zi = pc[3 * ii + 2];
        const float sqi = sq3(xi, yi, zi), kv = kth[pt];
        for (int j = 0; j < n; ++j) {
            const float xj = pc[3 * j], yj = pc[3 * j + 1], zj = pc[3 * j + 2];
            if (neg_sq_dist(sqi, xi, yi, zi, xj, yj, zj, sq3(xj, yj, zj)) >= kv) add(z4[(size_t)(cloud_base + j) * 16 + q]);
        }
    }
    return make_float4(acc.x / kdiv, acc.y / kdiv, acc.z / kdiv, acc.w / kdiv);
}
