/* epcnet_revisits.h -- revisit search: for every submap of a trajectory the k nearest descriptors among the submaps that lie at least
 * `min_travel` behind it -- the loop-closure candidates: the sixth header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from epcnet.h, epcnet_poses.h, epcnet_scans.h, epcnet_submaps.h and epcnet_stamps.h.  The entries carry the prefix
 * epcnet_: epcnet.h stays the complete list of the library's epc_ symbols.  This header is the first to pass a `double` by value.
 */
#ifndef EPCNET_REVISITS_H
#define EPCNET_REVISITS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Revisits: "where on this drive have I been before?" -- csrc/revisit.hip; numpy restatement: tests/revisit_ref.py */
/* ------------------------------------------------------------------------------------------------------ */
/* Submaps of one trajectory overlap, so the nearest descriptors of a submap are itself and its neighbours in time.  This entry is the
 * exact k-nearest search of the workspace form of the pairwise search in epcnet.h with a PER-QUERY ADMISSIBLE PREFIX of the database:
 * query i may only be answered by database rows that lie at least `min_travel` behind it along the trajectory.
 *
 * Inputs, in DEVICE memory and read when the kernels run:
 *   database (num_db, dim) float32, queries (num_q, dim) float32: descriptors, 16-byte aligned.  They may be the same buffer (a
 *       trajectory searched against itself), and queries may be rows of database (the streaming form).
 *   db_along (num_db) FLOAT64, q_along (num_q) FLOAT64: travelled distance in metres of every row (what ops.travel_along or
 *       k * spacing gives), or any other non-decreasing key, such as seconds for an exclusion by time.  db_along must be finite and
 *       non-decreasing; q_along may come in any order.
 * By value: min_travel (double, finite, >= 0), k, pass_queries.
 *
 * The admissible prefix.  For query i
 *     p_i = #{ j < num_db : db_along[j] <= fl(q_along[i] - min_travel) }
 * -- ONE float64 subtraction, rounded once, and a float64 comparison.  db_along is non-decreasing, so the admissible set is the prefix
 * database[:p_i]; in numpy: np.searchsorted(db_along, q_along - min_travel, side="right"), and that is the whole restatement.  With
 * min_travel > 0 and the trajectory searched against itself p_i <= i: the search is causal and every revisit pair is reported once, by
 * its later member.  min_travel == 0 admits the query's own row.
 *
 * The answer.  idx (num_q, k) int32 and dist (num_q, k) float32: row i holds the k nearest rows of database[:p_i], nearest first, and is
 * bit for bit what the pairwise search returns for the database database[:p_i], the one query queries[i] and min(k, p_i) neighbours: the
 * same sequential float32 sum_c (q_c - d_c)^2 and the same sqrtf; ties go to the lower index; a row or a query with a NaN or Inf
 * descriptor (the descriptor of a flagged submap) is never selected and selects nothing; (-1, +Inf) fills every position with no finite
 * neighbour -- the positions >= p_i included, and the whole row when p_i == 0.
 * count (num_q) int32: count[i] = p_i, or -1 where query i has no answer by rule: q_along[i] is not finite, or the whole call failed.
 * A query with count -1 has the row (-1, +Inf).
 *
 * Whole-call failure, decided on the device: db_along holds a non-finite entry or decreases anywhere.  Then EVERY count is -1, every idx
 * -1, every dist +Inf, and nothing else is written.  There is no status bit for it: count == -1 is the flag.
 *
 * Nothing is read back to the host: num_db, num_q, k and dim are host integers; the along values and the descriptors are read when the
 * kernels run, so the call is capturable in a graph and the graph replays on other data.  No memset on `stream`; the call writes every
 * word it later reads.
 *
 * How: a prepare step (row norms; one workgroup checks db_along and takes the largest finite database norm; one binary search per query
 * in float64 and the largest p of every tile of 128 queries), then per pass of `pass_queries` queries the tiled f32-MFMA distance GEMM
 * -- a workgroup whose database tile starts at or beyond its query tile's largest p returns at once: a sorted self-search computes half
 * the square --, per query the selection of k + 8 candidates over row[:p_i] only, their exact re-rank and the proof that no other row of
 * the prefix can belong (the proof's norm bound is the largest finite norm of the WHOLE database, which bounds every prefix), and the
 * exact redo of the rare query without proof.  Queries with p_i <= 0 write their row and never touch the matrix.  The matrix row
 * stride is num_db: the host cannot know the largest p without reading it back, so the triangle saves work, not workspace.
 *
 * pass_queries: the number of queries whose distance matrix is resident at once.  0 = the library's choice (the largest multiple of
 * 128 that keeps pass_queries * num_db * 4 bytes below 1 GiB, at least 128); otherwise a multiple of 128 in [128, 2^22].  The answer
 * does not depend on it.
 *
 * EPC_EINVAL, with nothing launched and nothing written, unless dim > 0 and dim % 8 == 0, 0 < k <= 56, 0 <= num_q <= 2^22,
 * 0 <= num_db <= 2^22, pass_queries is as above, min_travel is finite and >= 0, every pointer is non-NULL, and database, queries and
 * the workspace are 16-byte aligned.  num_q == 0 returns EPC_OK with nothing launched; num_db == 0 is valid (every row (-1, +Inf),
 * every count 0, or -1 for a non-finite q_along).  EPC_ENOMEM for a workspace shorter than
 * epcnet_revisit_workspace_bytes(num_db, num_q, pass_queries), which launches nothing and returns 0 for arguments the entry refuses.
 *
 * Not covered: geometric verification of a candidate pair, grouping consecutive hits into one closure, a distance threshold (the
 * caller thresholds dist), approximate or quantised indices, symmetric (non-causal) exclusion. */
size_t epcnet_revisit_workspace_bytes(int num_db, int num_q, int pass_queries);
int epcnet_revisit_search(const float* database, const double* db_along, int num_db, const float* queries, const double* q_along, int num_q,
                          int dim, double min_travel, int k, int pass_queries, int32_t* idx, float* dist, int32_t* count, void* workspace,
                          size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_REVISITS_H */
