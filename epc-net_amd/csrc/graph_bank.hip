// Cloud bank (include/epcnet.h, "Cloud bank"): the training set resident in HBM as one fixed-size record per cloud -- the cloud in
// Hilbert order together with its finished kNN graph (lists, transposed lists, overflow list) -- and the kernel that assembles a
// training step's batch from a list of record ids.  The sort, the neighbour lists and their transposition are functions of one
// cloud's coordinates alone (utils/tf_util.py:647-666; neighbours never cross clouds), the reference trains on the unaugmented
// preloaded submaps (train.py:228-230, :388) and revisits them every epoch: the step need not rebuild them.
//
//   epc_bank_record_bytes   size of one record (0 = unsupported shape)
//   epc_bank_store          what epc_morton_sort -> epc_knn_topk -> epc_knn_transpose + epc_knn_overflow_lists leave for a batch of
//                           clouds -> records (16-bit cloud-local indices; refused, never truncated, when a value does not fit)
//   epc_bank_assemble       ids (device) -> the batch tensors in exactly the layout the training kernels read (32-bit, re-based)
//   epc_bank_gather_infer   ids (device) -> what the inference pipeline holds after its sort and kNN launches (16-bit lists as stored)
//
// Record of a cloud of n points, cap slots per list (n % 8 == 0, cap % 8 == 0), in 16-byte chunks, every section 16-byte aligned:
//   chunk 0           int32 {ovf_cnt, rlist_used, n, cap}
//   xyz               n x 3 f32   Hilbert-sorted coordinates
//   kth, cnt, rdeg    n f32 / i32 / i32
//   roff              n i32       relative to the cloud's segment (absolute roff - c n cap)
//   idx               n x cap u16 cloud-local; the slots past min(cnt, cap) hold 0
//   rlist             n x cap u16 cloud-local (absolute row - c n); the entries past rlist_used hold 0
//   ovf               n u16       the overflow list; the entries past ovf_cnt hold 0
// 16 + 158 n bytes at cap = 32: 647,184 B for a 4096-point cloud against 1,179,652 B of the 32-bit tensors.
//
// The assemble kernel is a pure byte mover: per 4096-point cloud it reads ~0.55 MB (the record without the unused tail of rlist, ~62 %
// of whose n cap slots are taken at 20 neighbours per point) and writes ~1.0 MB.  18 clouds = ~28 MB; at the 6.3 TB/s a float4 copy
// reaches on this chip (8 TB/s HBM3E) that is 4.5 us, so the launch is bound by its ~2 us boundary as much as by its bytes.  One
// thread moves one 16-byte chunk per iteration: a dwordx4 load, and for the u16 sections the widening in registers and two dwordx4
// stores.  The grid is (slabs, T) with slabs chosen by the host so that T x slabs is ~4 workgroups per CU at any T.
#include "train_common.h"

namespace {

constexpr int BANK_THREADS = 256;

struct BankLayout {      // first chunk of every section, in 16-byte chunks from the start of the record
    unsigned xyz, kth, cnt, rdeg, roff, idx, rlist, ovf, end;
};

__host__ __device__ inline BankLayout bank_layout(int n, int cap) {
    BankLayout L;
    const unsigned q = (unsigned)n / 4, e = (unsigned)n * (unsigned)cap / 8;
    L.xyz = 1;
    L.kth = L.xyz + 3 * q;
    L.cnt = L.kth + q;
    L.rdeg = L.cnt + q;
    L.roff = L.rdeg + q;
    L.idx = L.roff + q;
    L.rlist = L.idx + e;
    L.ovf = L.rlist + e;
    L.end = L.ovf + (unsigned)n / 8;
    return L;
}

inline bool bank_shape_ok(int n, int cap) {
    return n >= 8 && n <= 65536 && n % 8 == 0 && cap >= EPC_KNN_SELECT && cap <= 64 && cap % 8 == 0;
}

struct BankTensors {     // the 32-bit batch tensors (store: inputs; assemble: outputs)
    float* xyz;          // (clouds, n, 3)
    float* kth;          // (clouds, n)
    int32_t* cnt;        // (clouds, n)
    int32_t* idx;        // (clouds, n, cap) cloud-local
    int32_t* rdeg;       // (clouds n)
    int32_t* roff;       // (clouds n) absolute: cloud c's lists start at c n cap
    int32_t* rlist;      // (clouds n cap) absolute rows
    int32_t* ovf_cnt;    // (clouds)
    int32_t* ovf_list;   // (clouds, n) cloud-local
};

__device__ __forceinline__ void widen8(const uint4 v, int add, int4& lo, int4& hi) {
    lo = make_int4((int)(v.x & 0xffffu) + add, (int)(v.x >> 16) + add, (int)(v.y & 0xffffu) + add, (int)(v.y >> 16) + add);
    hi = make_int4((int)(v.z & 0xffffu) + add, (int)(v.z >> 16) + add, (int)(v.w & 0xffffu) + add, (int)(v.w >> 16) + add);
}

// ---- assemble: grid (slabs, T); workgroup (slab, t) moves the chunks slab * 256 + tid, + slabs * 256, ... of record ids[t] ------------
__global__ __launch_bounds__(BANK_THREADS) void bank_assemble_kernel(const uint4* __restrict__ bank, long rec_chunks, int num_records,
                                                                     const int32_t* __restrict__ ids, int n, int cap, BankTensors o,
                                                                     int32_t* __restrict__ status, float* __restrict__ poison) {
    const int t = blockIdx.y, T = gridDim.y;
    const int id = ids[t];
    const bool bad = id < 0 || id >= num_records;
    const BankLayout L = bank_layout(n, cap);
    // the sticky status: bit (t & 31) of word t / 32 for every slot with an id outside the bank.  ONE workgroup forms whole words from
    // all the ids (a read-modify-write by one thread per word: no atomics, and no other workgroup of this launch touches them)
    if (blockIdx.x == 0 && t == 0) {
        for (int w = threadIdx.x; w * 32 < T; w += BANK_THREADS) {
            unsigned bits = 0;
            for (int b = 0; b < 32 && w * 32 + b < T; ++b) {
                const int v = ids[w * 32 + b];
                if (v < 0 || v >= num_records) bits |= 1u << b;
            }
            if (bits) status[w] = (int32_t)((unsigned)status[w] | bits);
        }
        // ... and THIS launch's verdict as a float the caller adds to its loss: 0 or NaN.  (NaN coordinates alone do not reach the
        // loss: the ReLUs and hinges downstream are fmaxf, which drops a NaN operand.)
        if (threadIdx.x == 0 && poison) {
            bool any = false;
            for (int u = 0; u < T; ++u) any = any || ids[u] < 0 || ids[u] >= num_records;
            *poison = any ? __builtin_nanf("") : 0.f;
        }
    }
    const size_t row0 = (size_t)t * n;                 // first row of slot t in the batch
    const int seg = t * n * cap;                       // first entry of slot t's rlist segment (the host checked T n cap < 2^31)
    const unsigned stride = gridDim.x * BANK_THREADS;
    if (bad) {
        // no record is read.  The slot gets NaN coordinates and an EMPTY, well-formed graph, so that no consumer follows an index
        // that was never written.
        const float qn = __builtin_nanf("");
        for (unsigned q = blockIdx.x * BANK_THREADS + threadIdx.x; q < L.rlist; q += stride) {
            if (q == 0) {
                o.ovf_cnt[t] = 0;
            } else if (q < L.kth) {
                reinterpret_cast<float4*>(o.xyz + row0 * 3)[q - L.xyz] = make_float4(qn, qn, qn, qn);
            } else if (q < L.cnt) {
                reinterpret_cast<float4*>(o.kth + row0)[q - L.kth] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else if (q < L.rdeg) {
                reinterpret_cast<int4*>(o.cnt + row0)[q - L.cnt] = make_int4(0, 0, 0, 0);
            } else if (q < L.roff) {
                reinterpret_cast<int4*>(o.rdeg + row0)[q - L.rdeg] = make_int4(0, 0, 0, 0);
            } else if (q < L.idx) {
                reinterpret_cast<int4*>(o.roff + row0)[q - L.roff] = make_int4(seg, seg, seg, seg);
            } else {
                int4* d = reinterpret_cast<int4*>(o.idx + row0 * cap) + 2 * (size_t)(q - L.idx);
                d[0] = make_int4(0, 0, 0, 0);
                d[1] = make_int4(0, 0, 0, 0);
            }
        }
        return;
    }
    const uint4* __restrict__ rec = bank + (size_t)id * rec_chunks;
    const int4 head = *reinterpret_cast<const int4*>(rec);             // {ovf_cnt, rlist_used, n, cap}: uniform over the workgroup
    const unsigned rlist_end = L.rlist + ((unsigned)head.y + 7) / 8, ovf_end = L.ovf + ((unsigned)head.x + 7) / 8;
    for (unsigned q = blockIdx.x * BANK_THREADS + threadIdx.x; q < L.end; q += stride) {
        if (q >= L.idx) {                                              // the 16-bit sections: 80 % of the chunks
            if (q < L.rlist) {
                int4 lo, hi;
                widen8(rec[q], 0, lo, hi);
                int4* d = reinterpret_cast<int4*>(o.idx + row0 * cap) + 2 * (size_t)(q - L.idx);
                d[0] = lo, d[1] = hi;
            } else if (q < L.ovf) {
                if (q < rlist_end) {                                   // (the unused tail of the segment is neither read nor written)
                    int4 lo, hi;
                    widen8(rec[q], (int)row0, lo, hi);
                    int4* d = reinterpret_cast<int4*>(o.rlist + seg) + 2 * (size_t)(q - L.rlist);
                    d[0] = lo, d[1] = hi;
                }
            } else if (q < ovf_end) {
                int4 lo, hi;
                widen8(rec[q], 0, lo, hi);
                int4* d = reinterpret_cast<int4*>(o.ovf_list + row0) + 2 * (size_t)(q - L.ovf);
                d[0] = lo, d[1] = hi;
            }
        } else if (q == 0) {
            o.ovf_cnt[t] = head.x;
        } else {
            uint4 v = rec[q];
            uint4* d;
            if (q < L.kth) d = reinterpret_cast<uint4*>(o.xyz + row0 * 3) + (q - L.xyz);
            else if (q < L.cnt) d = reinterpret_cast<uint4*>(o.kth + row0) + (q - L.kth);
            else if (q < L.rdeg) d = reinterpret_cast<uint4*>(o.cnt + row0) + (q - L.cnt);
            else if (q < L.roff) d = reinterpret_cast<uint4*>(o.rdeg + row0) + (q - L.rdeg);
            else {
                d = reinterpret_cast<uint4*>(o.roff + row0) + (q - L.roff);
                v.x += (unsigned)seg, v.y += (unsigned)seg, v.z += (unsigned)seg, v.w += (unsigned)seg;
            }
            *d = v;
        }
    }
}

// ---- gather for inference: grid (slabs, T); the sections the inference pipeline reads, as they are stored ------------------------------
// sorted xyz, kth, cnt and the u16 neighbour lists of record ids[t] -> slot t of the inference workspace: 5 n / 4 + n cap / 8 chunks per
// cloud, each read once and written once (4096 points at cap = 32: 344 KB each way, against ~0.55 MB in and ~1.0 MB out of the assemble
// kernel: no rdeg / roff / rlist / ovf, nothing widened).  The workgroups (0, t) additionally form slot t's status word from the record's
// coordinates with the test the kNN kernel applies to them ((x x + y y) + z z finite), so the word is written whole by one thread: no
// atomics, and the conv1 launch that follows may OR its EPC_STATUS_FP16_RANGE into it.
__global__ __launch_bounds__(BANK_THREADS) void bank_gather_infer_kernel(const uint4* __restrict__ bank, long rec_chunks, int num_records,
                                                                         const int32_t* __restrict__ ids, int n, int cap,
                                                                         float* __restrict__ xyz, float* __restrict__ kth,
                                                                         int32_t* __restrict__ cnt, unsigned short* __restrict__ idx,
                                                                         int32_t* __restrict__ status) {
    const int t = blockIdx.y;
    const int id = ids[t];
    const BankLayout L = bank_layout(n, cap);
    const uint4* __restrict__ rec = bank + (size_t)(id < 0 || id >= num_records ? 0 : id) * rec_chunks;
    bool bad = id < 0 || id >= num_records;
    if (!bad) {   // a record of another shape (a bank built for other clouds) is no record of this call either
        const int4 head = *reinterpret_cast<const int4*>(rec);
        bad = head.z != n || head.w != cap;
    }
    const size_t row0 = (size_t)t * n;
    const unsigned q4 = (unsigned)n / 4, low = 5 * q4, total = low + (L.rlist - L.idx);
    const unsigned stride = gridDim.x * BANK_THREADS;
    uint4* __restrict__ dx = reinterpret_cast<uint4*>(xyz + row0 * 3);
    uint4* __restrict__ dk = reinterpret_cast<uint4*>(kth + row0);
    uint4* __restrict__ dc = reinterpret_cast<uint4*>(cnt + row0);
    uint4* __restrict__ di = reinterpret_cast<uint4*>(idx + row0 * cap);
    if (bad) {
        // no record is read: NaN coordinates, an empty graph whose every list entry is row 0, and the status of a non-finite cloud
        const unsigned qn = 0x7fc00000u;
        for (unsigned p = blockIdx.x * BANK_THREADS + threadIdx.x; p < total; p += stride) {
            if (p < 3 * q4) dx[p] = make_uint4(qn, qn, qn, qn);
            else if (p < 4 * q4) dk[p - 3 * q4] = make_uint4(0, 0, 0, 0);
            else if (p < low) dc[p - 4 * q4] = make_uint4(0, 0, 0, 0);
            else di[p - low] = make_uint4(0, 0, 0, 0);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) status[t] = EPC_STATUS_NONFINITE_INPUT;
        return;
    }
    for (unsigned p = blockIdx.x * BANK_THREADS + threadIdx.x; p < total; p += stride) {
        if (p < 3 * q4) dx[p] = rec[L.xyz + p];
        else if (p < 4 * q4) dk[p - 3 * q4] = rec[L.kth + (p - 3 * q4)];
        else if (p < low) dc[p - 4 * q4] = rec[L.cnt + (p - 4 * q4)];
        else di[p - low] = rec[L.idx + (p - low)];
    }
    if (blockIdx.x == 0) {
        // thread u takes the points 4 u .. 4 u + 3 (three chunks), + 1024, ...
        bool nonfinite = false;
        for (unsigned u = threadIdx.x; u < q4; u += BANK_THREADS) {
            const uint4 a = rec[L.xyz + 3 * u], b = rec[L.xyz + 3 * u + 1], c = rec[L.xyz + 3 * u + 2];
            const float f[12] = {__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w),
                                 __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w),
                                 __uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w)};
#pragma unroll
            for (int j = 0; j < 4; ++j) nonfinite |= !(sq3(f[3 * j], f[3 * j + 1], f[3 * j + 2]) <= 3.4028234664e38f);
        }
        const int any = __syncthreads_or(nonfinite);
        if (threadIdx.x == 0) status[t] = any ? EPC_STATUS_NONFINITE_INPUT : 0;
    }
}

// ---- store, pass 1: does every meaningful value of the batch fit its record?  status[0] = 1 otherwise (plain stores of one value) ------
// Checked per cloud c: cnt in [0, n]; the first min(cnt, cap) entries of every idx row in [0, n); the transposed lists PACKED in point
// order inside the cloud's segment as epc_knn_transpose leaves them (roff[0] = c n cap, roff[j + 1] = roff[j] + rdeg[j], rdeg >= 0, the
// total <= n cap); every listed row inside the cloud; ovf_cnt in [0, n] and its entries in [0, n).  n <= 65536 (checked by the host) then
// bounds every stored index by 16 bits.
__global__ __launch_bounds__(BANK_THREADS) void bank_validate_kernel(int n, int cap, BankTensors s, int32_t* __restrict__ status) {
    const int c = blockIdx.y;
    const size_t row0 = (size_t)c * n;
    const long seg = (long)c * n * cap;
    bool ok = true;
    const int oc = s.ovf_cnt[c];
    ok = ok && oc >= 0 && oc <= n;
    const int last_off = s.roff[row0 + n - 1], last_deg = s.rdeg[row0 + n - 1];
    const long used = (long)last_off - seg + last_deg;
    ok = ok && last_deg >= 0 && used >= 0 && used <= (long)n * cap;
    for (int j = blockIdx.x * BANK_THREADS + threadIdx.x; j < n; j += gridDim.x * BANK_THREADS) {
        const int cn = s.cnt[row0 + j];
        ok = ok && cn >= 0 && cn <= n;
        const int m = cn < 0 ? 0 : (cn < cap ? cn : cap);
        for (int u = 0; u < m; ++u) {
            const int v = s.idx[(row0 + j) * cap + u];
            ok = ok && v >= 0 && v < n;
        }
        const int deg = s.rdeg[row0 + j];
        const long off = s.roff[row0 + j];
        ok = ok && deg >= 0 && (j == 0 ? off == seg : off == (long)s.roff[row0 + j - 1] + s.rdeg[row0 + j - 1]);
        if (j < oc && oc <= n) {
            const int v = s.ovf_list[row0 + j];
            ok = ok && v >= 0 && v < n;
        }
    }
    if (used >= 0 && used <= (long)n * cap)
        for (long p = blockIdx.x * BANK_THREADS + threadIdx.x; p < used; p += gridDim.x * BANK_THREADS) {
            const long v = (long)s.rlist[seg + p] - (long)row0;
            ok = ok && v >= 0 && v < n;
        }
    if (!ok) status[0] = 1;
}

// ---- store, pass 2 (nothing when pass 1 refused): one thread forms one 16-byte chunk of the record of cloud c -------------------------
__device__ __forceinline__ unsigned pack2(int a, int b) { return ((unsigned)a & 0xffffu) | ((unsigned)b << 16); }

__global__ __launch_bounds__(BANK_THREADS) void bank_store_kernel(uint4* __restrict__ bank, long rec_chunks, int first_slot, int n, int cap,
                                                                  BankTensors s, const int32_t* __restrict__ status) {
    if (status[0] != 0) return;
    const int c = blockIdx.y;
    const BankLayout L = bank_layout(n, cap);
    const size_t row0 = (size_t)c * n;
    const int seg = c * n * cap;
    const int oc = s.ovf_cnt[c];
    const int used = s.roff[row0 + n - 1] - seg + s.rdeg[row0 + n - 1];
    uint4* __restrict__ rec = bank + (size_t)(first_slot + c) * rec_chunks;
    for (unsigned q = blockIdx.x * BANK_THREADS + threadIdx.x; q < L.end; q += gridDim.x * BANK_THREADS) {
        uint4 v;
        if (q == 0) {
            v = make_uint4((unsigned)oc, (unsigned)used, (unsigned)n, (unsigned)cap);
        } else if (q < L.kth) {
            v = reinterpret_cast<const uint4*>(s.xyz + row0 * 3)[q - L.xyz];
        } else if (q < L.cnt) {
            v = reinterpret_cast<const uint4*>(s.kth + row0)[q - L.kth];
        } else if (q < L.rdeg) {
            v = reinterpret_cast<const uint4*>(s.cnt + row0)[q - L.cnt];
        } else if (q < L.roff) {
            v = reinterpret_cast<const uint4*>(s.rdeg + row0)[q - L.rdeg];
        } else if (q < L.idx) {
            v = reinterpret_cast<const uint4*>(s.roff + row0)[q - L.roff];
            v.x -= (unsigned)seg, v.y -= (unsigned)seg, v.z -= (unsigned)seg, v.w -= (unsigned)seg;
        } else {
            int e[8];
            const unsigned first = (q < L.rlist ? q - L.idx : q < L.ovf ? q - L.rlist : q - L.ovf) * 8u;
            if (q < L.rlist) {                          // eight slots of one idx row (cap % 8 == 0): zeros past min(cnt, cap)
                const unsigned j = first / (unsigned)cap, u0 = first % (unsigned)cap;
                const int cn = s.cnt[row0 + j];
                const int4* src = reinterpret_cast<const int4*>(s.idx + row0 * cap + first);
                const int4 a = src[0], b = src[1];
                const int raw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = (int)u0 + u < cn ? raw[u] : 0;
            } else if (q < L.ovf) {                     // eight entries of the packed transposed lists: zeros past `used`
                const int4* src = reinterpret_cast<const int4*>(s.rlist + seg + first);
                int raw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if ((int)first < used) {
                    const int4 a = src[0], b = src[1];
                    raw[0] = a.x, raw[1] = a.y, raw[2] = a.z, raw[3] = a.w, raw[4] = b.x, raw[5] = b.y, raw[6] = b.z, raw[7] = b.w;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = (int)first + u < used ? raw[u] - (int)row0 : 0;
            } else {
                int raw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if ((int)first < oc) {
                    const int4* src = reinterpret_cast<const int4*>(s.ovf_list + row0 + first);
                    const int4 a = src[0], b = src[1];
                    raw[0] = a.x, raw[1] = a.y, raw[2] = a.z, raw[3] = a.w, raw[4] = b.x, raw[5] = b.y, raw[6] = b.z, raw[7] = b.w;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = (int)first + u < oc ? raw[u] : 0;
            }
            v = make_uint4(pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7]));
        }
        rec[q] = v;
    }
}

inline bool tensors_ok(const BankTensors& b) {
    return b.xyz && b.kth && b.cnt && b.idx && b.rdeg && b.roff && b.rlist && b.ovf_cnt && b.ovf_list && epc_aligned16(b.xyz) &&
           epc_aligned16(b.kth) && epc_aligned16(b.cnt) && epc_aligned16(b.idx) && epc_aligned16(b.rdeg) && epc_aligned16(b.roff) && epc_aligned16(b.rlist) &&
           epc_aligned16(b.ovf_list);
}

// workgroups per cloud: ~4 per CU over the whole batch, at least 256 chunks each
inline unsigned bank_slabs(int clouds, unsigned chunks) {
    const unsigned want = (4u * (unsigned)epc_device_cu_count() + (unsigned)clouds - 1) / (unsigned)clouds;
    const unsigned most = (chunks + BANK_THREADS - 1) / BANK_THREADS;
    return want < 1 ? 1 : (want > most ? most : want);
}

}  // namespace

extern "C" size_t epc_bank_record_bytes(int n, int cap) {
    return bank_shape_ok(n, cap) ? (size_t)bank_layout(n, cap).end * 16 : 0;
}

extern "C" int epc_bank_store(void* bank, int num_records, int first_slot, int num_clouds, int n, int cap, const float* xyz_sorted,
                              const float* kth, const int32_t* cnt, const int32_t* idx, const int32_t* rdeg, const int32_t* roff,
                              const int32_t* rlist, const int32_t* ovf_cnt, const int32_t* ovf_list, int32_t* status, void* stream) {
    EPC_CHECK_ARG(bank_shape_ok(n, cap), "unsupported record shape (n a multiple of 8 in [8, 65536], cap a multiple of 8 in [20, 64])");
    EPC_CHECK_ARG(bank && status && epc_aligned16(bank), "null / unaligned bank or status");
    EPC_CHECK_ARG(num_clouds > 0 && first_slot >= 0 && num_records > 0 && (long)first_slot + num_clouds <= (long)num_records,
                  "slots outside the bank");
    EPC_CHECK_ARG((long)num_clouds * n * cap < (1L << 31), "too many edges for 32-bit offsets");
    BankTensors s{const_cast<float*>(xyz_sorted), const_cast<float*>(kth),     const_cast<int32_t*>(cnt),
                  const_cast<int32_t*>(idx),      const_cast<int32_t*>(rdeg),  const_cast<int32_t*>(roff),
                  const_cast<int32_t*>(rlist),    const_cast<int32_t*>(ovf_cnt), const_cast<int32_t*>(ovf_list)};
    EPC_CHECK_ARG(tensors_ok(s), "null / unaligned tensor");
    const BankLayout L = bank_layout(n, cap);
    const dim3 grid(bank_slabs(num_clouds, L.end), (unsigned)num_clouds);
    hipLaunchKernelGGL(bank_validate_kernel, grid, dim3(BANK_THREADS), 0, (hipStream_t)stream, n, cap, s, status);
    hipLaunchKernelGGL(bank_store_kernel, grid, dim3(BANK_THREADS), 0, (hipStream_t)stream, reinterpret_cast<uint4*>(bank), (long)L.end,
                       first_slot, n, cap, s, status);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

extern "C" int epc_bank_assemble(const void* bank, int num_records, const int32_t* ids, int num_ids, int n, int cap, float* xyz,
                                 float* kth, int32_t* cnt, int32_t* idx, int32_t* rdeg, int32_t* roff, int32_t* rlist, int32_t* ovf_cnt,
                                 int32_t* ovf_list, int32_t* status, float* poison, void* stream) {
    EPC_CHECK_ARG(bank_shape_ok(n, cap), "unsupported record shape (n a multiple of 8 in [8, 65536], cap a multiple of 8 in [20, 64])");
    EPC_CHECK_ARG(bank && ids && status && epc_aligned16(bank) && num_records > 0, "null / unaligned bank, ids or status");
    EPC_CHECK_ARG(num_ids > 0 && num_ids <= 65535 && (long)num_ids * n * cap < (1L << 31), "bad number of ids");
    BankTensors o{xyz, kth, cnt, idx, rdeg, roff, rlist, ovf_cnt, ovf_list};
    EPC_CHECK_ARG(tensors_ok(o), "null / unaligned tensor");
    const BankLayout L = bank_layout(n, cap);
    hipLaunchKernelGGL(bank_assemble_kernel, dim3(bank_slabs(num_ids, L.end), (unsigned)num_ids), dim3(BANK_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const uint4*>(bank), (long)L.end, num_records, ids, n, cap, o, status, poison);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

extern "C" int epc_bank_gather_infer(const void* bank, int num_records, const int32_t* ids, int num_ids, int n, int cap, float* xyz,
                                     float* kth, int32_t* cnt, void* idx_u16, int32_t* status, void* stream) {
    EPC_CHECK_ARG(bank_shape_ok(n, cap), "unsupported record shape (n a multiple of 8 in [8, 65536], cap a multiple of 8 in [20, 64])");
    EPC_CHECK_ARG(bank && ids && status && epc_aligned16(bank) && num_records > 0, "null / unaligned bank, ids or status");
    EPC_CHECK_ARG(num_ids > 0 && num_ids <= 65535, "bad number of ids");
    EPC_CHECK_ARG(xyz && kth && cnt && idx_u16 && epc_aligned16(xyz) && epc_aligned16(kth) && epc_aligned16(cnt) && epc_aligned16(idx_u16),
                  "null / unaligned tensor");
    const BankLayout L = bank_layout(n, cap);
    const unsigned moved = 5 * ((unsigned)n / 4) + (L.rlist - L.idx);
    hipLaunchKernelGGL(bank_gather_infer_kernel, dim3(bank_slabs(num_ids, moved), (unsigned)num_ids), dim3(BANK_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const uint4*>(bank), (long)L.end, num_records, ids, n, cap, xyz, kth, cnt,
                       reinterpret_cast<unsigned short*>(idx_u16), status);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}
