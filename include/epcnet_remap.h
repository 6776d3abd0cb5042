/* epcnet_remap.h -- rows TAKEN OUT of the surfel map that grows across calls, and rows RE-POSED in it (a later loop closure corrects
 * the poses their clouds were added at), at a cost that follows the rows moved and not the size of the map: the fourteenth header of
 * libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others (one row of its table of headers).  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols.
 */
#ifndef EPCNET_REMAP_H
#define EPCNET_REMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* "close the loops, then move the submaps the closure corrected to where they belong" --                   */
/* csrc/growmap.hip; numpy restatement: tests/remap_ref.py                                                   */
/* ------------------------------------------------------------------------------------------------------ */
/* epcnet_surfel_map_move works on the state, the six arrays and num_out of epcnet_growmap.h, under that header's rules: the same
 * origin, params and max_voxels, the same table, numbers and epochs, the same whole-call refusals.  The state's layout is unchanged.
 * It is possible because of what that header states: a slot's moments are integer sums, so a row is taken out by adding the two's-
 * complement negation of what it added (unsigned wrap-around; any interleaving of puts and take-outs gives the same sums); a voxel's
 * number never moves; a surfel depends on the cells within `ring` of its voxel only.
 *
 * THE CONTRACT.  After epcnet_surfel_map_init and ANY sequence of epcnet_surfel_map_add and epcnet_surfel_map_move calls, every voxel
 * whose count is > 0 holds in the six arrays, BIT FOR BIT, what epcnet_map_surfels (epcnet_surfels.h) writes for that cell over THE ROWS
 * CURRENTLY IN THE MAP AT THEIR CURRENT POSES, support included.  Voxels are matched by CELL: the numbers differ, because a number
 * handed out stays, and voxels that lost all their rows keep theirs.  num_out[1..3] are the rows currently in the map by kind under
 * their current poses (kept, absent, out of range): the head's counters go down as well as up.
 *
 * A ROW r of [offsets[0], offsets[num_clouds]), of cloud c.  Its OLD kind and lattice position are what epcnet_surfel_map_add computes
 * for it at old_poses[c], its NEW ones at new_poses[c] -- the same float64 sequence, the same origin and voxel.  With new_poses == NULL
 * (REMOVE) a row has no new kind.
 *   1. UNMOVED.  A row kept under both poses with identical lattice coordinates on all three axes touches nothing: no atomic, no epoch,
 *      nothing dirtied, nothing counted.  This test comes first: such a row is not looked up.
 *   2. UNMATCHED.  Else, if the old kind is kept and the row's old cell is not a voxel THAT EXISTED BEFORE THIS CALL, the row is skipped
 *      entirely -- not taken out, not put in, no row counter changed -- and counted in num_call[3].  (A cell that a row of this same
 *      call opens is not yet a voxel for this test, whatever the order the rows are worked in: the decision is deterministic.  A voxel
 *      that is empty still exists.)  A call cannot tell a row that was added from one that was not when its old cell is a voxel: taking
 *      a row out of an existing voxel that never held it is OUTSIDE THE CONTRACT, and still memory-safe -- sums wrap, no count is divided
 *      by when it is 0, every index is bounded, and a pool skips a cell whose count is below min_count, so a wrong count does not spread.
 *   3. TAKEN OUT.  Else, a row whose old kind is kept leaves the voxel of its old cell: count, the three 12-bit sums, A and B lose what
 *      the row added.  A row whose old kind is absent or out of range was never in a voxel: nothing is taken out for it.  Either way
 *      the head's row counter of the old kind falls by one.
 *   4. PUT IN.  A row of step 3 whose new kind is kept enters the voxel of its new cell exactly as an add puts it in (the cell is
 *      claimed where the table does not hold it), and is counted in num_call[1]; a row whose new kind is absent or out of range is only
 *      counted.  Either way the head's row counter of the new kind rises by one.  REMOVE has no step 4.
 * A row that moves inside one voxel (another lattice position, the same cell) is taken out of and put into the same slot.
 *
 * NEW VOXELS are numbered as an add numbers them: the cells this call claimed, by the lowest row put into each, behind the V the call
 * found.  EMPTY VOXELS: a voxel whose count reaches 0 keeps its slot and its number.  Its count is 0, its map_points, centroid,
 * normal and eigen are 0x7fc00000, and its support is the pooled N the shared solve returns (the cells within `ring` that hold at least
 * min_count rows).  Rows it receives later find the same voxel under the same number.  num_out[0] counts the numbered voxels, empty
 * ones included, and so does the capacity: overflow is still `slots claimed > max_voxels`, sticky, reported as an add reports it -- every
 * word of the arrays 0x7fc00000 / 0 from ONE call on, num_out[0] == -1; the row counters go on under the rules above against the voxels
 * numbered before the overflow.  Compaction is epcnet_surfel_map_init and adds.
 *
 * DIRTY VOXELS are those within `ring` (on every axis; a cell out of range is skipped, never wrapped) of a cell that had a row taken out
 * or put in by this call.  A move writes their rows of the six arrays and nothing else of them, and num_out.  A call whose rows are all
 * unmoved writes no row of the arrays.
 *
 * A REFUSED call -- invalid offsets (epcnet_maps.h), params or max_voxels that differ in any bit from init's, a state init never wrote
 * -- CHANGES NOTHING: not the state, not the arrays, not num_out; decided on the device, only num_call says so.
 *
 * size_t epcnet_surfel_map_move_workspace_bytes(num_rows, num_clouds, ring): the per-call scratch -- 8 bytes per row (the two slots),
 * 4 bytes per 256 rows, and the dirty list of 8 (2 ring + 1)^3 bytes per row -- sized from the call alone; 0 unless 0 <= num_rows <
 * 2^31, 0 <= num_clouds <= 2^24 and 0 <= ring <= EPC_SURFEL_MAX_RING.
 *
 * epcnet_surfel_map_move -- points, offsets, num_rows, num_clouds: the clouds as they were added (DEVICE memory); old_poses: (num_clouds,
 * 12) doubles, the poses they are in the map at; new_poses: the poses they move to, or NULL: remove.  old_poses == NULL is EPC_EINVAL:
 * that is epcnet_surfel_map_add.  params (HOST memory), max_voxels, state, the six arrays and num_out: as epcnet_surfel_map_add.
 *   num_call (4) int32, written by every call:
 *       [0] voxels new in this call; -1: the call numbered nothing -- it was refused on the device (then [1], [2], [3] are 0), or the map
 *           has overflowed (num_out[0] == -1)
 *       [1] rows put in
 *       [2] voxels whose outputs this call wrote (the dirty voxels)
 *       [3] rows unmatched
 * At most eight launches and no memset on `stream`, every one sized from num_rows, num_clouds and ring alone; nothing is read back.
 * Capturable: a captured graph replays on other points, offsets and poses of the same shape against the same state (params,
 * max_voxels and whether new_poses is NULL are part of the capture).  Integer atomics only.  EPC_EINVAL, with nothing launched and
 * nothing written, under the rules of epcnet_surfel_map_add; EPC_ENOMEM for a state shorter than epcnet_surfel_map_state_bytes(
 * max_voxels) or a workspace shorter than epcnet_surfel_map_move_workspace_bytes(num_rows, num_clouds, ring).
 *
 * Not covered: compaction of empty voxels; the localisation index of epcnet_localize.h patched in place (it is rebuilt from the arrays);
 * moving the origin; ray-casting (free space). */
size_t epcnet_surfel_map_move_workspace_bytes(long long num_rows, int num_clouds, int ring);
int epcnet_surfel_map_move(const float* points, const int32_t* offsets, long long num_rows, int num_clouds, const double* old_poses,
                           const double* new_poses, const double* params, long long max_voxels, void* state, size_t state_bytes,
                           float* map_points, int32_t* count, float* centroid, float* normal, float* eigen, int32_t* support,
                           int32_t* num_out, int32_t* num_call, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_REMAP_H */
