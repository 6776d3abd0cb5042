/* epcnet_localize.h -- scan-to-map localisation: point-to-plane ICP of Q scans against the surfel map of epcnet_surfels.h, and the
 * information of every estimate: the twelfth header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others (one row of its table of headers).  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols.  No `double` is passed by value: every scalar real goes in a `params` array in HOST memory, as
 * epcnet_map_surfels takes it.  The per-scan status bits are EPC_STATUS_NO_PAIR and EPC_STATUS_NO_FIT of epcnet_pairs.h.
 */
#ifndef EPCNET_LOCALIZE_H
#define EPCNET_LOCALIZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPC_LOCALIZE_INDEX_PARAMS 4
#define EPC_LOCALIZE_PARAMS 8

/* ------------------------------------------------------------------------------------------------------ */
/* The index: "which surfel lives in this cell?" -- csrc/localize.hip; numpy restatement:                    */
/* tests/localize_ref.py (index_reference)                                                                   */
/* ------------------------------------------------------------------------------------------------------ */
/* Built ONCE per map and reused by every epcnet_scan_localize call on it: a streaming caller does not rebuild it per scan.
 *
 * Inputs, in DEVICE memory and read when the kernels run:
 *   anchor (M, 3) float32: the point that names a surfel's cell.  Pass epcnet_map_surfels' map_points: the voxel's own mean, which lies
 *       in or on the face of its own cell (the centroid is pooled over neighbouring cells and may lie in another one).
 *   centroid (M, 3), normal (M, 3) float32: epcnet_map_surfels' outputs.  The caller filters: a surfel it does not want (not flat
 *       enough, too little support) gets a NaN word in its normal before the call.
 *   params: FOUR doubles in HOST memory, read during the call: voxel, 0, 0, 0.  voxel in [2^-20, 2^20].
 *
 * THE DEFINITION.  Surfel j is PRESENT iff its nine words (anchor, centroid, normal) are all finite.  Its cell is
 *     k_a = floor(fl((double)anchor_a / voxel)),  a = 0, 1, 2
 * and it is OUT OF RANGE unless every k_a lies in [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL) (epcnet_maps.h).  The float32 rounding of
 * map_points can put the anchors of two voxels into one cell (a mean just below a face rounds onto it): among the present surfels in
 * range of one cell the LOWEST j is INDEXED (an integer minimum: the same on every run), the others are DUPLICATES.
 *
 * Outputs:
 *   index: index_bytes >= epcnet_surfel_index_bytes(M) bytes of device memory, 16-byte aligned, whose layout is private to the two
 *       entries.  The call writes every byte of the first epcnet_surfel_index_bytes(M) (a launch, not a memset); it records M and voxel.
 *   num (4) int32: surfels indexed, not present, duplicates, out of range; they add up to M.
 *
 * Four launches, no memset, nothing read back: capturable, and the graph replays on another map of the same M.  Integer atomics only.
 * The index is an open-addressing table of the smallest power of two >= 2 M + 1 slots of 32 bytes (an empty slot always exists), 4
 * bytes more per slot while it is built, and 128 bytes in front.
 * EPC_EINVAL, with nothing launched and nothing written, unless 1 <= M <= 2^28, voxel is as above, the three reserved doubles are 0,
 * every pointer is non-NULL and index is 16-byte aligned; EPC_ENOMEM for index_bytes < epcnet_surfel_index_bytes(M), which returns 0
 * for an M outside the range. */
size_t epcnet_surfel_index_bytes(long long M);
int epcnet_surfel_index(const float* anchor, const float* centroid, const float* normal, long long M, const double* params, void* index,
                        size_t index_bytes, int32_t* num, void* stream);

/* ------------------------------------------------------------------------------------------------------ */
/* Localisation: "where is this scan in the map, and how well is that known?" -- csrc/localize.hip; numpy     */
/* restatement: tests/localize_ref.py (localize_reference)                                                    */
/* ------------------------------------------------------------------------------------------------------ */
/* Inputs, in DEVICE memory and read when the kernels run:
 *   scans (Q, n, 3) float32 in METRES, 16-byte aligned (what the down-sampler returns without its normalisation).  A row with a
 *       non-finite word is ABSENT.  n is a multiple of 32 in [32, 4096].
 *   seeds (Q, H, 12) FLOAT64: row-major [R | t] hypotheses that map a scan into the map's frame RELATIVE TO THE MAP'S ORIGIN (the
 *       frame of centroid); NULL = one seed per scan, the identity (H must then be 1).  H in [1, 64].
 *   index, index_bytes: what epcnet_surfel_index built for this map; centroid, normal (M, 3), M: the arrays it was built from.  The
 *       index holds the words of every indexed surfel, taken when it was built; a map whose arrays change is indexed again.
 *   params: EIGHT doubles in HOST memory, read during the call: voxel, max_dist, iterations, min_pairs, 0, 0, 0, 0.  voxel: the
 *       index's; max_dist finite and > 0; iterations an integer value in [0, 64]; min_pairs an integer value in [6, n].
 * An index that does not record this M and this voxel (another map's, or never built) flags EVERY scan EPC_STATUS_NO_PAIR; it is
 * not followed.
 *
 * THE DEFINITION.  Every floating-point operation below is rounded once (no fused multiply-add), written fl(.) where it matters; the
 * only operations are + - * /, floor, the correctly rounded square root and comparisons.  Float64 unless stated.
 *
 * Transform.  Under a pose m[12] = [R | t], for every row that is not absent, (x, y, z) its float32 words:
 *     r_c = (m[4c] * x + m[4c + 1] * y) + m[4c + 2] * z          the row rotated about the sensor
 *     p_c = (float)(r_c + m[4c + 3]),   c = 0, 1, 2               its place in the map, rounded once more to float32.
 *
 * Correspondence.  The row's cell is k_a = floor(fl((double)p_a / voxel)).  Its CANDIDATES are the indexed surfels of the 27 cells
 * k + o, o in [-1, 1]^3, in the order 9 (o_2 + 1) + 3 (o_1 + 1) + (o_0 + 1).  A cell counts iff k_a + o_a lies in
 * [-EPC_MAP_MAX_CELL, EPC_MAP_MAX_CELL) on every axis: a cell outside the range is skipped, never wrapped (a row whose k_a is not
 * finite has no candidate).  With c the candidate's CENTROID, in float32,
 *     d2 = (dx * dx + dy * dy) + dz * dz,   dx = p_0 - c_0, dy = p_1 - c_1, dz = p_2 - c_2
 * where a d2 that is NaN counts as +Inf.  The row takes the candidate with the smallest d2, ties to the lower order, and is ACCEPTED iff
 *     d2 <= gate2,  gate2 = min((float)(max_dist * max_dist), FLT_MAX), the product formed in double
 * (epcnet_pairs.h; gate2 is finite: a row without a candidate is never accepted).  Candidates come from the 27 cells only: a max_dist
 * above voxel reaches no further.
 *
 * Residual and Jacobian of an accepted row, in float64 from the float32 words p, c and the candidate's normal n:
 *     e  = (n_0 * (p_0 - c_0) + n_1 * (p_1 - c_1)) + n_2 * (p_2 - c_2)
 *     J0 = r_1 * n_2 - r_2 * n_1     J1 = r_2 * n_0 - r_0 * n_2     J2 = r_0 * n_1 - r_1 * n_0          (r x n)
 *     J3 = n_0                       J4 = n_1                       J5 = n_2
 * the derivative of e under R <- C(omega) R, t <- t + v at delta = (omega, v) = 0.  Linearising about the sensor position (r, not
 * p) keeps kilometre-sized map coordinates out of the 6 x 6 matrix.
 *
 * Sums.  Over the accepted rows, 29 float64 sums: [0] the count (leaves 1.0); [1 .. 21] J_i * J_j for i <= j in the order 00 01 02 03
 * 04 05 11 12 .. 55; [22 + i] J_i * e; [28] e * e; every leaf one rounded product.  The ORDER of summation is epcnet_pairs.h's: 4096
 * leaves indexed by the scan's row; an absent row, a row that is not accepted and every row >= n is the leaf +0.0; the leaves are
 * combined by adjacent pairing until one is left,
 *     while len(v) > 1: v = v[0::2] + v[1::2]
 *
 * Solve.  H[i][j] = H[j][i] = sums[1 ..], b[i] = sums[22 + i]; delta = the solution of H delta = -b by the unpivoted Cholesky exactly
 * as epcnet_trajectory.h writes it, with r[i] = -b[i]:
 *     for j = 0..5:  s = H[j][j];  for k = 0..j-1: s = s - L[j][k] * L[j][k];   a pivot s that is not > 0 FAILS;   L[j][j] = sqrt(s)
 *                    for i = j+1..5:  s = H[i][j];  for k = 0..j-1: s = s - L[i][k] * L[j][k];   L[i][j] = s / L[j][j]
 *     for i = 0..5:  s = r[i];  for k = 0..i-1: s = s - L[i][k] * y[k];   y[i] = s / L[i][i]
 *     for i = 5..0:  s = y[i];  for k = i+1..5: s = s - L[k][i] * delta[k];   delta[i] = s / L[i][i]
 * With (w, x, y, z) = (1, 0.5 * delta_0, 0.5 * delta_1, 0.5 * delta_2), C the rotation of that unnormalised quaternion by the formula
 * of epcnet_stamps.h (nn = ((w*w + x*x) + y*y) + z*z, u = 2 / nn, C00 = 1 - u * (y*y + z*z), C01 = u * (x*y - w*z), ...) and
 * d3(a, b) = (a0 * b0 + a1 * b1) + a2 * b2 as in epcnet_trajectory.h:
 *     R[i][j] <- d3(C i:, R :j);    t[i] <- t[i] + delta[3 + i].     Nothing is renormalised.
 * A failed pivot, or a new pose that holds a non-finite word, ends the scan with EPC_STATUS_NO_FIT.
 *
 * Stage A, the seed: one pass per seed without a non-finite word.  The best seed has the largest count; ties go to the smaller
 * sums[28], then to the lower seed index.  No such seed: EPC_STATUS_NO_PAIR.
 * Stage B, refinement: `iterations` times from the best seed: pass, then solve; no convergence test.  A pass with fewer than min_pairs
 * accepted rows ends the scan with EPC_STATUS_NO_FIT.  (The first pass of stage B is the best seed's pass of stage A.)
 * Final pass: one more pass under the result (with iterations == 0: under the best seed).  Fewer than min_pairs accepted rows here
 * is EPC_STATUS_NO_FIT too.
 *
 * Outputs -- the call writes every word of all five:
 *   pose (Q, 12) float64: [R | t], scan into the map's frame -- the last solve's, or the best seed's own words with iterations == 0.
 *   fit (Q, 2) float64: sums[28] / sums[0] of the final pass (the mean squared point-to-plane residual, metres squared) and sums[0] /
 *       (rows that are not absent).
 *   hessian (Q, 21) float64: sums[1 .. 21] of the final pass, the upper triangle of sum J J^T in the order above: the information of
 *       the estimate in (rad, m) about the sensor, up to the caller's sigma^-2.  A direction the map does not constrain -- along a
 *       corridor, or in a single plane -- is a near-null direction of this matrix.
 *   info (Q, 4) int32: the best seed, sums[0] of the final pass, the rows that are not absent, 0.
 *   status (Q) int32: 0, EPC_STATUS_NO_PAIR or EPC_STATUS_NO_FIT.
 * A flagged scan (either bit) has a NaN pose (0x7ff8000000000000), a NaN fit, a NaN hessian, best seed -1 and 0 accepted rows; its
 * row count stays.
 *
 * What converges to what.  The centroid of a surfel is formed from floors on a lattice of voxel / 256 (epcnet_surfels.h): it lies
 * BELOW the mean of its rows by less than voxel / 256 on every axis.  On a scene of exact planes with unit normals n_k, a row of plane
 * k at the true pose has the residual n_k . (mean - centroid) up to the float32 rounding of p, c and n: less than |n_k|_1 voxel / 256
 * <= sqrt(3) voxel / 256 in magnitude and of one sign per axis -- a bias, not noise.  To first order and with the rotation held, the
 * translation settles where N dt = b, N the matrix of three planes' normals by rows and |b_k| < sqrt(3) voxel / 256:
 *     |dt| < 3 voxel / 256 * |N^-1|_2        (2.3 mm at 0.2 m for orthogonal planes; a floor's mean bias is half a step per axis,
 *                                             so about a quarter of it is what to expect)
 * The coupling with the rotation has no bound as clean.  tests/test_localize_cpu.py holds the restatement's translation to this bound
 * and its rotation to twice what the restatement itself leaves on that scene; both numbers are written there.
 *
 * Nothing is read back to the host and every grid is sized from the arguments alone, so the call is capturable in a graph and the
 * graph replays on other scans, seeds and another map of the same M indexed into the same buffer (params are part of the capture).
 * No memset on `stream`, no atomics; no kernel reads a workspace word that an earlier kernel of the same call has not written.
 *
 * How: one launch counts the rows of every scan and checks its seeds and the index; a correspondence launch per pass -- grid (scan,
 * seed, chunk of 256 rows), one row per lane, 27 hashed lookups of one 32-byte slot each, the chunk's 29 subtree sums written to the
 * workspace -- and a solve launch behind each that finishes the tree, chooses the seed or solves, and after the final pass writes
 * the outputs (2 * iterations + 3 launches).
 *
 * EPC_EINVAL, with nothing launched and nothing written, unless n % 32 == 0 and 32 <= n <= 4096, 0 <= Q <= 2^20, 1 <= H <= 64 (1
 * where seeds is NULL), 1 <= M <= 2^28, voxel in [2^-20, 2^20], max_dist is finite and > 0, iterations and min_pairs are as above, the
 * four reserved doubles are 0, every pointer but seeds is non-NULL, and scans, index and the workspace are 16-byte aligned.  Q == 0
 * returns EPC_OK with nothing launched.  EPC_ENOMEM for index_bytes < epcnet_surfel_index_bytes(M) or a workspace shorter than
 * epcnet_scan_localize_workspace_bytes(Q, H, n), which launches nothing and returns 0 for arguments the entry refuses.
 *
 * Not covered: robust kernels beyond the gate; point-to-plane with scan-side normals, symmetric or GICP metrics; NDT; an index patched in
 * place when the map grows (epcnet_growmap.h: it is built again); candidate rings other than 1; global localisation without a seed. */
size_t epcnet_scan_localize_workspace_bytes(int Q, int H, int n);
int epcnet_scan_localize(const float* scans, int Q, int n, const double* seeds, int H, const void* index, size_t index_bytes,
                         const float* centroid, const float* normal, long long M, const double* params, double* pose, double* fit,
                         double* hessian, int32_t* info, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_LOCALIZE_H */
