// The surfel map that grows across calls (include/epcnet_growmap.h: epcnet_surfel_map_init, epcnet_surfel_map_add; numpy restatement in
// tests/growmap_ref.py).  The definition is epcnet_map_surfels' on the concatenation of the calls' clouds, and so is the code: the claim
// loop, the lookup and the scan's levels are map_common.h's, the slot, a tile's rows, the sixteen-lane adds and the pool-and-solve
// surfel_common.h's, here on a table that persists in the caller's state.  What an add has to do beyond the sums follows from three
// facts: a voxel's number is its first source row's rank, so numbers handed out never move; the sums are integers, free of how rows were
// split over calls; a surfel depends on the cells within `ring` of its voxel only.  So a call numbers the slots it claimed behind the V
// it found, and solves again the voxels within `ring` of a slot that received a row -- the DIRTY ones -- and no other.
//
// The state: a head (gm_head, 256 bytes) | the table (mp_cap(max_voxels) slots of 128 bytes).  A slot's last two words carry its leader (a
// row of the call that claimed it), its number + 1 (0: not numbered yet) and two epochs: the call in which it last received a row, the call
// in which it was last marked dirty.  The head's epoch is the number of the call in progress: 1 after init, incremented at the end of every
// call that was not refused, on the device -- a replayed graph advances it.  Epochs are compared for equality, never with 0 or <.
//
// offsets, poses, the origin and the epoch are device data: every grid of an add is sized from num_rows, num_clouds and ring alone.
//   scan_clear_words        clears the workspace's head (scan_common.h: a launch, not a memset)
//   growmap_check_kernel    the whole-call failure: the offsets' rule; the head's magic, max_voxels and the bits of the eight params
//   growmap_insert_kernel   surfel_insert_kernel on the persistent table.  The atomicMin on the leader applies to slots without a number:
//                           an old slot keeps its number, whatever its stale leader says.  The first row of this call to reach a slot wins
//                           an atomicExch of the epoch into `touched`; it notes so in bit 30 of its row_slot word (a slot index is < 2^30)
//   growmap_mark_kernel     tiles over the rows, behind the insert (every key of this call is in the table): the tile's count of leaders
//                           -- rows that lead a slot without a number --, then every winner looks up the (2 ring + 1)^3 cells around
//                           its slot (out of range: skipped, never wrapped) and exchanges the epoch into `dirty` of each that is a voxel;
//                           whoever flips one appends the slot to the dirty list through an integer counter.  The list's order varies
//                           from run to run; the outputs are written by voxel number, so it does not reach them
//   growmap_group_kernel, growmap_top_kernel     the scan's upper levels (map_common.h); V, num_out, num_call, the epoch's increment,
//                           and whether this call has to fill the outputs after an overflow (the first such call does, once)
//   growmap_number_kernel   tiles over the rows: every leader writes V_before + its rank + 1 into its slot
//   growmap_emit_kernel     lanes over the dirty list, the grid sized from min(num_rows (2 ring + 1)^3, max_voxels); lanes behind the
//                           count leave.  A lane writes map_points and count from its slot and the nine words and support from
//                           sf_pool_solve, at its slot's number: nothing else of the outputs is written.  After an overflow: the fill, a
//                           loop of this grid over max_voxels, in one call only
// Overflow is `claimed > max_voxels`, as in surfel.hip; claimed lives in the head and never falls, so it is sticky by itself.
//
// epcnet_surfel_map_move (include/epcnet_remap.h; numpy restatement in tests/remap_ref.py) takes rows out of the map and puts them back
// at other poses on the same state: the sums are integers, so a row leaves by the negation of what it added.  Its launches are add's
// with ONE other tile kernel in the place of the insert:
//   growmap_move_kernel     a tile's rows under both poses (sf_tile_row twice).  A row kept under both at the same lattice position
//                           leaves here.  The old cell is looked up, never claimed: a slot without a number was claimed in this call
//                           (numbers are written behind this launch), so "a voxel that existed before this call" is `found and
//                           numbered` in whatever order the rows run -- a row that fails it is unmatched and does nothing more.  The
//                           new cell is claimed as the insert claims it.  Both slots take the epoch into `touched`; row_slot is two
//                           words per row, [2 r] the slot left and [2 r + 1] the slot entered, each with its GM_WON; two rounds of
//                           the sixteen-lane adds, the first negated.  The head's three row counters move by the tile's signed sums
// The mark kernel walks every word of a row (ws.per_row: 1 for add, 2 for move), the leaders are read from a row's LAST word (the slot
// it entered), and the dirty list holds per_row times as many entries; the scan, the numbers and the emit are the same launches.  A
// voxel that lost its last row keeps slot and number: the emit writes count 0 and NaN for it (sf_write_mean divides by no zero count).
// Integer atomics only, no inline assembly, no scratch.
#include "surfel_common.h"
#include "../../include/epcnet_growmap.h"
#include "../../include/epcnet_remap.h"

#define GM_MAGIC 0x3170616d776f7267ull      // "growmap1": a state that init wrote
#define GM_WON (1 << 30)                    // in a row_slot word >= 0: this row was its slot's first of the call
// the workspace's head beyond MP_BAD and MP_KEPT .. MP_KEPT + 2 (this call's rows kept, absent, out of range)
#define GM_DIRTY 5                          //   [5] entries of the dirty list
#define GM_VBASE 6                          //   [6] V before this call
#define GM_FILL 7                           //   [7] this call fills the outputs after an overflow
#define GM_UNMATCHED 8                      //   [8] a move's rows whose old cell was no voxel before the call (an add leaves it 0)
// a move keeps in [MP_KEPT] its rows put in, and in [MP_KEPT + 1], [MP_KEPT + 2] nothing: the head's counters take the signed sums

struct gm_head {
    unsigned long long magic;
    long long max_voxels;
    double origin[3];
    unsigned long long params[EPC_SURFEL_PARAMS];      // the bits of init's eight doubles
    uint32_t epoch;                // the call in progress
    int32_t claimed;               // slots claimed: MP_CLAIMED of surfel.hip's head
    int32_t numbered;              // V
    int32_t kept[3];               // rows kept, absent, out of range: cumulative
    int32_t filled;                // the outputs were filled after the overflow
    int32_t pad[31];
};
static_assert(sizeof(gm_head) == EPC_GROWMAP_HEAD_BYTES, "the head is what the header says");
static_assert(EPC_GROWMAP_HEAD_BYTES % 128 == 0, "a slot is one 128-byte line of an aligned state");

struct gm_bits { unsigned long long w[EPC_SURFEL_PARAMS]; };

struct gm_state {
    gm_head* head;
    sf_slot* table;
    unsigned long long mask;       // cap - 1
};
struct gm_state_layout_t { gm_state st; size_t bytes; };
static gm_state_layout_t gm_state_layout(void* state, long long max_voxels) {
    epc_carver c(state);
    const unsigned long long cap = mp_cap(max_voxels);
    return {{c.take<gm_head>(1), c.take<sf_slot>(cap), cap - 1}, c.bytes()};
}

// the workspace: head (16 int32, padded to 128 bytes) | row_slot (num_rows int32) | tile counts | group totals | the dirty list
// (num_rows (2 ring + 1)^3 int32: every winner appends at most that many), each rounded up to 16 bytes.  A move has per_row = 2 words of
// row_slot per row -- the slot left, the slot entered -- and so twice the dirty list
struct gm_ws {
    int32_t* head;
    int32_t* row_slot;
    int32_t* tile;
    int32_t* group;
    int32_t* dirty;
    long long dirty_cap;
    int per_row;
};
struct gm_layout_t { gm_ws ws; size_t bytes; };
static gm_layout_t gm_layout(void* workspace, long long num_rows, int ring, int per_row = 1) {
    epc_carver c(workspace);
    const long long side = 2 * ring + 1, cap = per_row * num_rows * side * side * side;
    return {{c.take<int32_t>(MP_HEAD, 128), c.take<int32_t>((size_t)(per_row * num_rows), 16), c.take<int32_t>((size_t)mp_tiles(num_rows), 16),
             c.take<int32_t>((size_t)mp_groups(num_rows), 16), c.take<int32_t>((size_t)cap, 16), cap, per_row}, c.bytes()};
}

// ---- init: the table, the head, the outputs of no row --------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void growmap_init_kernel(const double* __restrict__ origin, gm_bits params, long long max_voxels,
                                                                  gm_state st, float* __restrict__ map_points, int32_t* __restrict__ count,
                                                                  float* __restrict__ centroid, float* __restrict__ normal,
                                                                  float* __restrict__ eigen, int32_t* __restrict__ support,
                                                                  int32_t* __restrict__ num_out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * MP_THREADS;
    const unsigned long long first = (unsigned long long)blockIdx.x * MP_THREADS + threadIdx.x;
    sf_clear_table(st.table, st.mask, first, stride);
    for (unsigned long long j = first; j < (unsigned long long)max_voxels; j += stride)
        sf_write_none((long long)j, map_points, count, centroid, normal, eigen, support);
    if (first < 4) num_out[first] = 0;
    if (first == 0) {
        gm_head* h = st.head;
        h->magic = GM_MAGIC;
        h->max_voxels = max_voxels;
        for (int a = 0; a < 3; ++a) h->origin[a] = origin[a];
        for (int e = 0; e < EPC_SURFEL_PARAMS; ++e) h->params[e] = params.w[e];
        h->epoch = 1;
        h->claimed = 0, h->numbered = 0, h->kept[0] = 0, h->kept[1] = 0, h->kept[2] = 0, h->filled = 0;
        for (int e = 0; e < 31; ++e) h->pad[e] = 0;
    }
}

// ---- add, launch 2: the whole-call failure ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void growmap_check_kernel(const int32_t* __restrict__ offsets, long long num_rows, int num_clouds,
                                                                   gm_bits params, long long max_voxels, gm_state st, gm_ws ws) {
    const long long i = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
    bool bad = i < (num_clouds > 0 ? num_clouds : 1) && offsets_rule_bad(offsets, num_clouds, num_rows, i);
    if (i == 0) {
        const gm_head* h = st.head;
        bad |= h->magic != GM_MAGIC || h->max_voxels != max_voxels;
        for (int e = 0; e < EPC_SURFEL_PARAMS; ++e) bad |= h->params[e] != params.w[e];
    }
    if (bad) atomicOr(&ws.head[MP_BAD], 1);
}

// ---- launch 3: the rows ----------------------------------------------------------------------------------------------------------------
// the epoch into a slot's `touched` -> this row is the slot's first of the call
__device__ __forceinline__ bool gm_touch(uint32_t* touched, uint32_t epoch) {
    return __atomic_load_n(touched, __ATOMIC_RELAXED) != epoch && atomicExch(touched, epoch) != epoch;
}
// row r enters slot t: its position for the tile's adds; its claim to lead, unless the slot has a number (claimed in an earlier call: it
// keeps its number, whatever its stale leader says); the epoch -> won
__device__ __forceinline__ bool gm_enter(sf_tile_lds& lds, int tid, sf_slot* table, int slot, long long r, const long long* w, uint32_t epoch) {
    sf_stage_pos(lds, tid, w);
    sf_slot* t = table + slot;
    if (mp_load(&t->number) == 0) sf_lead(t, r);
    return gm_touch(&t->touched, epoch);
}

__global__ __launch_bounds__(MP_THREADS) void growmap_insert_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                    long long num_rows, int num_clouds, const double* __restrict__ poses,
                                                                    sf_params pr, long long max_voxels, gm_state st, gm_ws ws) {
    __shared__ sf_tile_lds lds;
    if (ws.head[MP_BAD]) return;                       // (uniform: the launch before this one decided it)
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * MP_TILE, r = r0 + tid;
    const uint32_t epoch = st.head->epoch;
    long long w[3];
    const int kind = sf_tile_row(points, offsets, num_rows, num_clouds, poses, st.head->origin, pr.voxel, lds, r0, w);
    int slot = -kind;                                  // -1 absent, -2 out of range, -4 no row of any cloud
    bool won = false;
    if (kind == 0) {
        slot = mp_claim(st.table, st.mask, mp_key(w[0] >> 12, w[1] >> 12, w[2] >> 12), &st.head->claimed, max_voxels);      // -3: gave up
        if (slot >= 0) won = gm_enter(lds, tid, st.table, slot, r, w, epoch);
    }
    if (r < num_rows) ws.row_slot[r] = won ? slot | GM_WON : slot;
    lds.slot[tid] = slot;
    __syncthreads();
    sf_add_rows(st.table, lds);
    __syncthreads();
    if (tid < 3 && lds.kinds[tid]) {
        atomicAdd(&ws.head[MP_KEPT + tid], lds.kinds[tid]);
        atomicAdd(&st.head->kept[tid], lds.kinds[tid]);
    }
}

// ---- a move's launch 3: the rows out of their old cells and into their new ones (include/epcnet_remap.h, steps 1 to 4) -----------------------
// new_poses == nullptr: remove -- no row has a new kind
__global__ __launch_bounds__(MP_THREADS) void growmap_move_kernel(const float* __restrict__ points, const int32_t* __restrict__ offsets,
                                                                  long long num_rows, int num_clouds, const double* __restrict__ old_poses,
                                                                  const double* __restrict__ new_poses, sf_params pr, long long max_voxels,
                                                                  gm_state st, gm_ws ws) {
    __shared__ sf_tile_lds out, in;                    // the rows taken out, the rows put in
    __shared__ int moved[5];                           // the tile's signed sums of the three kinds; rows put in; rows unmatched
    if (ws.head[MP_BAD]) return;                       // (uniform: the launch before this one decided it)
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * MP_TILE, r = r0 + tid;
    const uint32_t epoch = st.head->epoch;
    if (tid < 5) moved[tid] = 0;                       // (sf_tile_row's barriers stand between this and the first add)
    long long wo[3], wn[3];
    const int ko = sf_tile_row(points, offsets, num_rows, num_clouds, old_poses, st.head->origin, pr.voxel, out, r0, wo);
    const int kn = new_poses ? sf_tile_row(points, offsets, num_rows, num_clouds, new_poses, st.head->origin, pr.voxel, in, r0, wn) : 4;
    int so = -1, sn = -1;
    bool won_o = false, won_n = false;
    const bool unmoved = ko == 0 && kn == 0 && wo[0] == wn[0] && wo[1] == wn[1] && wo[2] == wn[2];
    if (ko != 4 && !unmoved) {
        bool matched = true;
        if (ko == 0) {                                 // found AND numbered: a slot claimed in this call has no number yet
            const long long at = mp_find(st.table, st.mask, mp_key(wo[0] >> 12, wo[1] >> 12, wo[2] >> 12));
            matched = at >= 0 && mp_load(&st.table[at].number) != 0;
            if (matched) so = (int)at;
        }
        if (!matched) {
            atomicAdd(&moved[4], 1);
        } else {
            atomicAdd(&moved[ko], -1);
            if (kn < 3) atomicAdd(&moved[kn], 1);
            if (kn == 0) {
                atomicAdd(&moved[3], 1);
                sn = mp_claim(st.table, st.mask, mp_key(wn[0] >> 12, wn[1] >> 12, wn[2] >> 12), &st.head->claimed, max_voxels);   // -3: gave up
            }
            if (so >= 0) {                             // (numbered: it has no leader to find)
                sf_stage_pos(out, tid, wo);
                won_o = gm_touch(&st.table[so].touched, epoch);
            }
            if (sn >= 0) won_n = gm_enter(in, tid, st.table, sn, r, wn, epoch);
        }
    }
    if (r < num_rows) {
        ws.row_slot[2 * r] = won_o ? so | GM_WON : so;
        ws.row_slot[2 * r + 1] = won_n ? sn | GM_WON : sn;
    }
    out.slot[tid] = so, in.slot[tid] = sn;
    __syncthreads();
    sf_add_rows<true>(st.table, out);
    sf_add_rows(st.table, in);
    __syncthreads();
    if (tid < 3 && moved[tid]) atomicAdd(&st.head->kept[tid], moved[tid]);
    if (tid == 3 && moved[3]) atomicAdd(&ws.head[MP_KEPT], moved[3]);
    if (tid == 4 && moved[4]) atomicAdd(&ws.head[GM_UNMATCHED], moved[4]);
}

// the call changes no voxel: it was refused, or more voxels than max_voxels were claimed (row_slot and the table may not be followed)
__device__ __forceinline__ bool gm_no_map(const gm_state& st, const gm_ws& ws, long long max_voxels) {
    return ws.head[MP_BAD] != 0 || (long long)st.head->claimed > max_voxels;
}

// row r leads a voxel that is new in this call: the slot it entered -- the last of its row_slot words -- has no number and names it the
// leader (a numbered slot's leader is stale)
__device__ __forceinline__ int gm_is_leader(const gm_state& st, const gm_ws& ws, long long r, long long num_rows, int* slot) {
    *slot = -1;
    if (r >= num_rows) return 0;
    const int s = ws.row_slot[r * ws.per_row + (ws.per_row - 1)];
    if (s < 0) return 0;
    *slot = s & (GM_WON - 1);
    const sf_slot* t = st.table + *slot;
    return mp_load(&t->number) == 0 && t->leader == (int)r ? 1 : 0;
}

// ---- launch 4: the tiles' leaders, and the dirty voxels -------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void growmap_mark_kernel(long long num_rows, int ring, long long max_voxels, gm_state st, gm_ws ws) {
    __shared__ int part[MP_THREADS / 64];
    if (gm_no_map(st, ws, max_voxels)) return;
    int slot, total;
    const long long r = (long long)blockIdx.x * MP_TILE + threadIdx.x;
    block_scan<MP_THREADS / 64, int>(gm_is_leader(st, ws, r, num_rows, &slot), part, total);
    if (threadIdx.x == 0) ws.tile[blockIdx.x] = total;
    if (r >= num_rows) return;
    const uint32_t epoch = st.head->epoch;
    for (int word = 0; word < ws.per_row; ++word) {    // an add's one slot; a move's slot left and slot entered
        const int s = ws.row_slot[r * ws.per_row + word];
        if (s < 0 || !(s & GM_WON)) continue;
        long long g0, g1, g2;
        mp_cell(st.table[s & (GM_WON - 1)].key, g0, g1, g2);
        for (int o2 = -ring; o2 <= ring; ++o2) {
            if (!mp_in_range(g2 + o2)) continue;
            for (int o1 = -ring; o1 <= ring; ++o1) {
                if (!mp_in_range(g1 + o1)) continue;
                for (int o0 = -ring; o0 <= ring; ++o0) {
                    if (!mp_in_range(g0 + o0)) continue;
                    const long long at = mp_find(st.table, st.mask, mp_key(g0 + o0, g1 + o1, g2 + o2));
                    if (at < 0) continue;
                    uint32_t* dp = &st.table[at].dirty;
                    // (one atomic add per flipped slot.  Lanes of a wave that flip in the same step sharing ONE add -- a ballot -- measured
                    // the same: 0.327 against 0.329 ms per add of 80 000 rows into an empty map, 0.811 against 0.818 ms into 1.43 M voxels)
                    if (__atomic_load_n(dp, __ATOMIC_RELAXED) != epoch && atomicExch(dp, epoch) != epoch) {
                        const int k = atomicAdd(&ws.head[GM_DIRTY], 1);
                        if ((long long)k < ws.dirty_cap) ws.dirty[k] = (int)at;    // (k < cap always: the bound only keeps a wrong count inside)
                    }
                }
            }
        }
    }
}

// ---- launches 5 to 7: every leader's number ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_GROUP) void growmap_group_kernel(long long tiles, long long max_voxels, gm_state st, gm_ws ws) {
    __shared__ int part[MP_GROUP / 64];
    if (gm_no_map(st, ws, max_voxels)) return;
    mp_scan_group(tiles, ws.tile, ws.group, part);
}

__global__ __launch_bounds__(MP_THREADS) void growmap_top_kernel(long long groups, long long max_voxels, gm_state st, gm_ws ws,
                                                                 int32_t* __restrict__ num_out, int32_t* __restrict__ num_call) {
    __shared__ int part[MP_THREADS / 64];
    const bool bad = ws.head[MP_BAD] != 0, over = (long long)st.head->claimed > max_voxels;
    int fresh = 0;
    if (!bad && !over) fresh = mp_scan_top(groups, ws.group, part);
    if (threadIdx.x != 0) return;
    if (bad) {                                         // the state and the outputs stay as they were
        num_call[0] = -1, num_call[1] = 0, num_call[2] = 0, num_call[3] = 0;
        return;
    }
    gm_head* h = st.head;
    const int before = h->numbered;
    if (!over) h->numbered = before + fresh;           // == claimed: every claimed slot has a leader
    ws.head[GM_VBASE] = before;
    ws.head[GM_FILL] = over && !h->filled ? 1 : 0;
    if (over) h->filled = 1;
    h->epoch += 1;                                     // the next call's (the launches behind this one do not read it)
    num_out[0] = over ? -1 : before + fresh;
    num_out[1] = h->kept[0], num_out[2] = h->kept[1], num_out[3] = h->kept[2];
    const int dirty = ws.head[GM_DIRTY];
    num_call[0] = over ? -1 : fresh;
    num_call[1] = ws.head[MP_KEPT];
    num_call[2] = over ? 0 : (long long)dirty < ws.dirty_cap ? dirty : (int)ws.dirty_cap;
    num_call[3] = ws.head[GM_UNMATCHED];               // (an add: the cleared word)
}

__global__ __launch_bounds__(MP_THREADS) void growmap_number_kernel(long long num_rows, long long max_voxels, gm_state st, gm_ws ws) {
    __shared__ int part[MP_THREADS / 64];
    if (gm_no_map(st, ws, max_voxels)) return;
    int slot, total;
    const int lead = gm_is_leader(st, ws, (long long)blockIdx.x * MP_TILE + threadIdx.x, num_rows, &slot);
    const int place = block_scan<MP_THREADS / 64, int>(lead, part, total);
    if (!lead) return;
    const long long j = (long long)ws.head[GM_VBASE] + ws.group[blockIdx.x / MP_GROUP] + ws.tile[blockIdx.x] + place;
    if (j < max_voxels) __atomic_store_n(&st.table[slot].number, (int32_t)(j + 1), __ATOMIC_RELAXED);      // (j < V <= max_voxels here)
}

// ---- launch 8: the outputs of the dirty voxels ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void growmap_emit_kernel(long long max_voxels, sf_params pr, gm_state st, gm_ws ws,
                                                                  float* __restrict__ map_points, int32_t* __restrict__ count,
                                                                  float* __restrict__ centroid, float* __restrict__ normal,
                                                                  float* __restrict__ eigen, int32_t* __restrict__ support) {
    if (ws.head[MP_BAD]) return;
    const long long i = (long long)blockIdx.x * MP_THREADS + threadIdx.x;
    if ((long long)st.head->claimed > max_voxels) {
        if (ws.head[GM_FILL])
            for (long long j = i; j < max_voxels; j += (long long)gridDim.x * MP_THREADS)
                sf_write_none(j, map_points, count, centroid, normal, eigen, support);
        return;
    }
    const long long listed = ws.head[GM_DIRTY];
    if (i >= listed || i >= ws.dirty_cap) return;
    const sf_slot* t = st.table + ws.dirty[i];
    const long long j = (long long)t->number - 1;
    if (j < 0 || j >= max_voxels) return;              // (0 <= j < V here: the bound only keeps a wrong number inside the buffers)
    sf_write_mean(t, pr, j, map_points, count);
    sf_write_surfel(st.table, st.mask, t, pr, j, centroid, normal, eigen, support);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
static gm_bits gm_bits_of(const double* params) {
    gm_bits b;
    for (int e = 0; e < EPC_SURFEL_PARAMS; ++e) __builtin_memcpy(&b.w[e], &params[e], 8);
    return b;
}

// the size queries answer 0 where the entries refuse: mp_shape_refusal's bounds, with a value in range for what a query does not take
extern "C" size_t epcnet_surfel_map_state_bytes(long long max_voxels) {
    if (!mp_supported(0, 0, max_voxels)) return 0;
    return gm_state_layout(nullptr, max_voxels).bytes;
}

static size_t gm_workspace_bytes(long long num_rows, int num_clouds, int ring, int per_row) {
    if (!mp_supported(num_rows, num_clouds, 1) || ring < 0 || ring > EPC_SURFEL_MAX_RING) return 0;
    return gm_layout(nullptr, num_rows, ring, per_row).bytes;
}
extern "C" size_t epcnet_surfel_map_add_workspace_bytes(long long num_rows, int num_clouds, int ring) {
    return gm_workspace_bytes(num_rows, num_clouds, ring, 1);
}
extern "C" size_t epcnet_surfel_map_move_workspace_bytes(long long num_rows, int num_clouds, int ring) {
    return gm_workspace_bytes(num_rows, num_clouds, ring, 2);
}

// the refusals of a state under the name of the entry `who` (init checks under its own; add and move share gm_call, which is told
// the entry's)
#define GM_STATE_REFUSALS(who, state, state_bytes, max_voxels)                                                \
    do {                                                                                                      \
        EPC_CHECK_ARG_AS(who, epc_aligned16(state), "state must be 16-byte aligned");                         \
        EPC_CHECK_BYTES_AS(who, "state", state_bytes, epcnet_surfel_map_state_bytes(max_voxels));             \
    } while (0)

extern "C" int epcnet_surfel_map_init(const double* origin, const double* params, long long max_voxels, void* state, size_t state_bytes,
                                      float* map_points, int32_t* count, float* centroid, float* normal, float* eigen, int32_t* support,
                                      int32_t* num_out, void* stream) {
    EPC_CHECK_ARG(origin && params && state && map_points && count && centroid && normal && eigen && support && num_out, "null pointer");
    const char* const shape = mp_shape_refusal(0, 0, max_voxels);
    EPC_CHECK_ARG(!shape, shape);
    const char* const refusal = sf_params_refusal(params);
    EPC_CHECK_ARG(!refusal, refusal);
    GM_STATE_REFUSALS(__func__, state, state_bytes, max_voxels);
    const gm_state st = gm_state_layout(state, max_voxels).st;
    hipLaunchKernelGGL(growmap_init_kernel, dim3(sf_clear_blocks(st.mask)), dim3(MP_THREADS), 0, (hipStream_t)stream, origin, gm_bits_of(params),
                       max_voxels, st, map_points, count, centroid, normal, eigen, support, num_out);
    EPC_CHECK_LAUNCH();
    return EPC_OK;
}

// add and move: the same refusals and the same launches around ONE tile kernel of their own -- the insert, or the move (then row_slot
// has two words per row and new_poses may be NULL: remove)
static int gm_call(const char* who, bool move, const float* points, const int32_t* offsets, long long num_rows, int num_clouds,
                   const double* poses, const double* new_poses, const double* params, long long max_voxels, void* state, size_t state_bytes,
                   float* map_points, int32_t* count, float* centroid, float* normal, float* eigen, int32_t* support, int32_t* num_out,
                   int32_t* num_call, void* workspace, size_t workspace_bytes, void* stream) {
    EPC_CHECK_ARG_AS(who, points && offsets && poses && params && state && map_points && count && centroid && normal && eigen && support &&
                              num_out && num_call && workspace,
                     "null pointer");
    const char* const shape = mp_shape_refusal(num_rows, num_clouds, max_voxels);
    EPC_CHECK_ARG_AS(who, !shape, shape);
    const char* const refusal = sf_params_refusal(params);
    EPC_CHECK_ARG_AS(who, !refusal, refusal);
    GM_STATE_REFUSALS(who, state, state_bytes, max_voxels);
    const sf_params pr = sf_params_of(params);
    const gm_layout_t layout = gm_layout(workspace, num_rows, pr.ring, move ? 2 : 1);
    EPC_CHECK_WORKSPACE_AS(who, workspace, workspace_bytes, layout.bytes);
    hipStream_t s = (hipStream_t)stream;
    const gm_state st = gm_state_layout(state, max_voxels).st;
    const gm_ws ws = layout.ws;
    const long long tiles = mp_tiles(num_rows), groups = mp_groups(num_rows);
    if (int rc = scan_clear_words_launch(ws.head, MP_HEAD, s, who)) return rc;
    const long long checks = num_clouds > 0 ? ((long long)num_clouds + MP_THREADS - 1) / MP_THREADS : 1;
    hipLaunchKernelGGL(growmap_check_kernel, dim3((unsigned)checks), dim3(MP_THREADS), 0, s, offsets, num_rows, num_clouds, gm_bits_of(params),
                       max_voxels, st, ws);
    EPC_CHECK_LAUNCH_AS(who);
    if (tiles > 0) {
        if (move)
            hipLaunchKernelGGL(growmap_move_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, s, points, offsets, num_rows, num_clouds, poses,
                               new_poses, pr, max_voxels, st, ws);
        else
            hipLaunchKernelGGL(growmap_insert_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, s, points, offsets, num_rows, num_clouds, poses,
                               pr, max_voxels, st, ws);
        EPC_CHECK_LAUNCH_AS(who);
        hipLaunchKernelGGL(growmap_mark_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, s, num_rows, pr.ring, max_voxels, st, ws);
        EPC_CHECK_LAUNCH_AS(who);
        hipLaunchKernelGGL(growmap_group_kernel, dim3((unsigned)groups), dim3(MP_GROUP), 0, s, tiles, max_voxels, st, ws);
        EPC_CHECK_LAUNCH_AS(who);
    }
    hipLaunchKernelGGL(growmap_top_kernel, dim3(1), dim3(MP_THREADS), 0, s, groups, max_voxels, st, ws, num_out, num_call);
    EPC_CHECK_LAUNCH_AS(who);
    if (tiles > 0) {
        hipLaunchKernelGGL(growmap_number_kernel, dim3((unsigned)tiles), dim3(MP_THREADS), 0, s, num_rows, max_voxels, st, ws);
        EPC_CHECK_LAUNCH_AS(who);
        // a call's dirty voxels: at most (2 ring + 1)^3 per slot that a row left or entered, and never more than the map holds
        const long long bound = ws.dirty_cap < max_voxels ? ws.dirty_cap : max_voxels;
        hipLaunchKernelGGL(growmap_emit_kernel, dim3((unsigned)((bound + MP_THREADS - 1) / MP_THREADS)), dim3(MP_THREADS), 0, s, max_voxels, pr,
                           st, ws, map_points, count, centroid, normal, eigen, support);
        EPC_CHECK_LAUNCH_AS(who);
    }
    return EPC_OK;
}

extern "C" int epcnet_surfel_map_add(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                                     const double* params, long long max_voxels, void* state, size_t state_bytes, float* map_points,
                                     int32_t* count, float* centroid, float* normal, float* eigen, int32_t* support, int32_t* num_out,
                                     int32_t* num_call, void* workspace, size_t workspace_bytes, void* stream) {
    return gm_call(__func__, false, points, offsets, num_rows, num_clouds, poses, nullptr, params, max_voxels, state, state_bytes, map_points,
                   count, centroid, normal, eigen, support, num_out, num_call, workspace, workspace_bytes, stream);
}

extern "C" int epcnet_surfel_map_move(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* old_poses,
                                      const double* new_poses, const double* params, long long max_voxels, void* state, size_t state_bytes,
                                      float* map_points, int32_t* count, float* centroid, float* normal, float* eigen, int32_t* support,
                                      int32_t* num_out, int32_t* num_call, void* workspace, size_t workspace_bytes, void* stream) {
    return gm_call(__func__, true, points, offsets, num_rows, num_clouds, old_poses, new_poses, params, max_voxels, state, state_bytes, map_points,
                   count, centroid, normal, eigen, support, num_out, num_call, workspace, workspace_bytes, stream);
}
