/* epcnet_growmap.h -- the surfel map that GROWS ACROSS CALLS: a persistent state on the device, an `add` whose work scales with the rows
 * added and not with the size of the map: the thirteenth header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others (one row of its table of headers).  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols.
 */
#ifndef EPCNET_GROWMAP_H
#define EPCNET_GROWMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* A map that grows: "localise a scan against the map, put it into the map, localise the next" --           */
/* csrc/growmap.hip; numpy restatement: tests/growmap_ref.py                                                 */
/* ------------------------------------------------------------------------------------------------------ */
/* THE CONTRACT.  After epcnet_surfel_map_init and ANY sequence of epcnet_surfel_map_add calls, the seven outputs -- map_points, count,
 * centroid, normal, eigen, support, num_out -- are BIT-EQUAL to what epcnet_map_surfels (epcnet_surfels.h) writes for the CONCATENATION
 * of those calls' clouds: each call's rows in [offsets[0], offsets[num_clouds]) in call order, the poses appended, at the same origin,
 * voxel, min_count, ring, min_support and max_voxels.  The three row counts of num_out are cumulative.  Nothing of that definition
 * changes:
 *   - voxels are numbered by their first source row, so a number handed out never moves when rows are appended;
 *   - the moments and the pooled sums are integers, so they do not depend on how the rows were split over calls;
 *   - a voxel's surfel depends on the cells within `ring` of it only.
 * After a call, the voxels within `ring` (on every axis) of a cell that RECEIVED a row in that call -- the DIRTY voxels -- are the only
 * ones whose outputs can differ in any bit: an add writes the rows of the dirty voxels in the six arrays and nothing else of them, and
 * num_out.
 *
 * Overflow: once the concatenation holds more than max_voxels voxels, every float word is 0x7fc00000, every count and support 0 and
 * num_out[0] == -1, on that call and on every later one (the row counts go on), exactly as the one-shot entry reports those inputs.
 * A call whose offsets are invalid (epcnet_maps.h), or whose params or max_voxels differ in any bit from what init recorded, or whose
 * state init never wrote, ADDS NOTHING: the state, the six arrays and num_out stay as they were, decided on the device; only num_call
 * says so.
 *
 * The state: a head of EPC_GROWMAP_HEAD_BYTES bytes, then the open-addressing table of epcnet_map_surfels -- the smallest power of two
 * >= 2 max_voxels + 1 slots of 128 bytes -- whose slots carry, besides the integer sums, the voxel's number and two 32-bit EPOCHS: the
 * call in which the slot last received a row and the call in which it was last marked dirty.  The epoch is a word of the head, 1 after init, that every
 * add which is not refused increments on the device -- a replayed graph advances it --; comparisons are for equality, so a state serves
 * 2^32 - 1 adds between two inits (the next one would carry the epoch of a cleared slot).  Everything in it is device data: the caller owns the bytes and
 * must not touch them between init and the last add.
 *
 * size_t epcnet_surfel_map_state_bytes(max_voxels): the bytes of a state; 0 unless 1 <= max_voxels <= 2^28.
 *
 * epcnet_surfel_map_init -- once per map, and again to empty it.  origin (3 doubles, DEVICE memory) and params (EPC_SURFEL_PARAMS
 * doubles in HOST memory, read during the call: voxel, min_count, ring, min_support, 0, 0, 0, 0 under the rules of epcnet_map_surfels)
 * are recorded in the head; the table is cleared; EVERY word of the six arrays is written (0x7fc00000 / 0) and num_out is 0, 0, 0, 0:
 * what epcnet_map_surfels writes for no row.  One launch; the only call whose work scales with max_voxels.  EPC_EINVAL with nothing
 * launched for a null pointer, a state that is not 16-byte aligned, max_voxels or params outside their rules; EPC_ENOMEM for state_bytes
 * < epcnet_surfel_map_state_bytes(max_voxels).
 *
 * size_t epcnet_surfel_map_add_workspace_bytes(num_rows, num_clouds, ring): the per-call scratch -- 4 bytes per row, 4 bytes per 256
 * rows, and the dirty list of 4 (2 ring + 1)^3 bytes per row -- sized from the call alone; 0 unless 0 <= num_rows < 2^31, 0 <=
 * num_clouds <= 2^24 and 0 <= ring <= EPC_SURFEL_MAX_RING.
 *
 * epcnet_surfel_map_add -- points, offsets, num_rows, num_clouds, poses: as epcnet_map_surfels (DEVICE memory); params (HOST memory)
 * and max_voxels: init's; the six arrays and num_out: the ones init wrote (the call relies on the rows it does not write).
 *   num_call (4) int32, written by every call:
 *       [0] voxels new in this call; -1: the call numbered nothing -- it was refused on the device (then [1] and [2] are 0), or the
 *           map has overflowed (num_out[0] == -1)
 *       [1] rows kept in this call
 *       [2] voxels whose outputs this call wrote (the dirty voxels)
 *       [3] 0
 * At most eight launches and no memset on `stream`, every one sized from num_rows, num_clouds and ring alone; nothing is read back.
 * Capturable: a captured graph replays on other points, offsets and poses of the same shape against the same state (params and
 * max_voxels are part of the capture).  Integer atomics only.  The order of the dirty list varies from run to run; the outputs are
 * written by voxel number, so it does not reach them.  After an overflow ONE call fills the six arrays (a loop of that call's grid over
 * max_voxels); later calls keep num_out only.  EPC_EINVAL, with nothing launched and nothing written, under the rules of
 * epcnet_map_surfels, for a null pointer and for a state or workspace that is not 16-byte aligned; EPC_ENOMEM for a state shorter than
 * epcnet_surfel_map_state_bytes(max_voxels) or a workspace shorter than epcnet_surfel_map_add_workspace_bytes(num_rows, num_clouds,
 * ring).
 *
 * Not covered: the localisation index of epcnet_localize.h patched in place (it is rebuilt from the arrays: a quarter of a millisecond
 * at 1.4 M voxels); moving the origin; ray-casting (free space).  Removing rows and re-posing rows after a later loop closure are
 * epcnet_remap.h's epcnet_surfel_map_move, on this state: a voxel it leaves without a row keeps slot and number, with count 0. */
#define EPC_GROWMAP_HEAD_BYTES 256
size_t epcnet_surfel_map_state_bytes(long long max_voxels);
int epcnet_surfel_map_init(const double* origin, const double* params, long long max_voxels, void* state, size_t state_bytes,
                           float* map_points, int32_t* count, float* centroid, float* normal, float* eigen, int32_t* support,
                           int32_t* num_out, void* stream);
size_t epcnet_surfel_map_add_workspace_bytes(long long num_rows, int num_clouds, int ring);
int epcnet_surfel_map_add(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* poses,
                          const double* params, long long max_voxels, void* state, size_t state_bytes, float* map_points, int32_t* count,
                          float* centroid, float* normal, float* eigen, int32_t* support, int32_t* num_out, int32_t* num_call,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_GROWMAP_H */
