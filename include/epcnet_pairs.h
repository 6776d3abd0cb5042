/* epcnet_pairs.h -- pair registration: the rigid alignment of P candidate pairs of clouds by point-to-point ICP from caller-given seed
 * poses, and how well each pair fits -- the geometric verification of a loop-closure candidate: the seventh header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from epcnet.h, epcnet_poses.h, epcnet_scans.h, epcnet_submaps.h, epcnet_stamps.h and epcnet_revisits.h.  The
 * entries carry the prefix epcnet_: epcnet.h stays the complete list of the library's epc_ symbols.  Like epcnet_revisits.h this header
 * passes a `double` by value.
 */
#ifndef EPCNET_PAIRS_H
#define EPCNET_PAIRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-pair status bits (bits 1 .. 128 belong to the earlier headers) */
#define EPC_STATUS_NO_PAIR 256 /* a cloud index outside [0, num_clouds), or no seed without a non-finite word */
#define EPC_STATUS_NO_FIT 512  /* a pass accepted fewer than min_pairs rows, or a solve gave a non-finite pose */

/* ------------------------------------------------------------------------------------------------------ */
/* Pairs: "is this candidate really the same place, and where am I relative to it?" -- csrc/register.hip; numpy restatement:
 * tests/register_ref.py */
/* ------------------------------------------------------------------------------------------------------ */
/* A descriptor match (epcnet_revisits.h) is a hypothesis.  This entry aligns the two clouds of every candidate pair and scores the
 * alignment, so that the caller can threshold the score and hand the relative pose to a pose graph.
 *
 * Inputs, in DEVICE memory and read when the kernels run:
 *   clouds (num_clouds, n, 3) float32 in METRIC units (what the down-sampler returns without its normalisation), 16-byte aligned.  A row
 *       with a non-finite word is ABSENT.  n is a multiple of 32 in [32, 4096].
 *   pairs (num_pairs, 2) int32: (source cloud, target cloud).
 *   seeds (num_pairs, num_seeds, 12) FLOAT64: row-major [R | t] hypotheses that map the source into the target; NULL = one seed per pair,
 *       the identity (num_seeds must then be 1).
 * By value: max_dist (double, finite, > 0), iterations in [0, 64], min_pairs in [3, n], num_seeds in [1, 64].
 *
 * THE DEFINITION.  Every floating-point operation below is rounded once (no fused multiply-add); the only operations are + - * /, the
 * correctly rounded square root and comparisons.
 *
 * Correspondence pass under a pose m[12] = [R | t].  For every source row i that is not absent, (x, y, z) its float32 words:
 *     p_c = (float)(((m[4c] * x + m[4c + 1] * y) + m[4c + 2] * z) + m[4c + 3]),  c = 0, 1, 2
 * in float64, rounded once more to float32.  Its nearest target row j minimises, over the target rows that are not absent, the float32
 *     d2 = (dx * dx + dy * dy) + dz * dz,   dx = p_0 - q_x, dy = p_1 - q_y, dz = p_2 - q_z
 * where a d2 that is NaN counts as +Inf; ties go to the lower row.  The correspondence (i, j) is ACCEPTED when d2 <= gate2,
 *     gate2 = min((float)(max_dist * max_dist), FLT_MAX), the product formed in double.
 * (gate2 is finite, so a row whose every d2 is +Inf -- an all-absent target, an overflowed p -- is never accepted.)
 *
 * Sums.  Over the accepted rows, 17 float64 sums: [0] the count (leaves 1.0), [1..3] sum s_a, [4..6] sum q_b, [7 + 3a + b] sum s_a * q_b,
 * [16] sum d2 -- s the ORIGINAL source row, q the target row, every leaf exact in float64.  The ORDER of summation is normative: 4096
 * leaves indexed by source row; an absent row, a rejected row and every row >= n is the leaf +0.0; the leaves are combined by adjacent
 * pairing until one is left,
 *     while len(v) > 1: v = v[0::2] + v[1::2]
 * (a lane-xor butterfly inside a wave, then the waves of a workgroup, then the workgroups of a pair: an aligned chunk of consecutive
 * rows is a subtree).
 *
 * Solve, from the 17 sums, m = sums[0]:
 *     M_ab = S_ab - (sum s_a * sum q_b) / m                                          (a over the source, b over the target)
 *     N00 = (Mxx + Myy) + Mzz   N01 = Myz - Mzy            N02 = Mzx - Mxz            N03 = Mxy - Myx
 *                               N11 = (Mxx - Myy) - Mzz    N12 = Mxy + Myx            N13 = Mzx + Mxz
 *                                                          N22 = (Myy - Mxx) - Mzz    N23 = Myz + Mzy
 *                                                                                     N33 = (Mzz - Mxx) - Myy
 * (Horn's symmetric matrix).  Its eigenvectors by cyclic Jacobi: A = N, V = I, then 6 sweeps over the pairs
 * (p, q) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3).  A pair with a_pq == 0 is skipped; otherwise
 *     theta = (a_qq - a_pp) / (2 * a_pq);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta * theta + 1))
 *     c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * a_pq
 *     a_pp -= h;  a_qq += h;  a_pq = a_qp = 0
 *     for r not in {p, q}:  g = a_rp, f = a_rq;  a_rp = a_pr = c * g - s * f;  a_rq = a_qr = s * g + c * f
 *     for r in 0..3:        g = v_rp, f = v_rq;  v_rp = c * g - s * f;         v_rq = s * g + c * f
 * 6 is the smallest count at which one more sweep moved no bit of the rotation, checked with tests/register_ref.py on the CPU: on the
 * scenes of tests/test_register_cpu.py and on 300,000 matrices whose largest eigenvalue is simple (random symmetric ones and Horn matrices
 * of noisy point sets; most settle after 4, 18 of them needed 6).  The quaternion (w, x, y, z) is
 * the column of V with the largest a_kk (ties: the lower k), UNNORMALISED; the rotation is built from it as epcnet_stamps.h does:
 *     nn = ((w*w + x*x) + y*y) + z*z;  u = 2 / nn
 *     R = [ 1 - u*(y*y + z*z)   u*(x*y - w*z)       u*(x*z + w*y)
 *           u*(x*y + w*z)       1 - u*(x*x + z*z)   u*(y*z - w*x)
 *           u*(x*z - w*y)       u*(y*z + w*x)       1 - u*(x*x + y*y) ]
 *     t_c = qm_c - ((R_c0 * sm_x + R_c1 * sm_y) + R_c2 * sm_z),   sm_a = sum s_a / m,  qm_b = sum q_b / m.
 * A solve whose pose holds a non-finite word ends the pair with EPC_STATUS_NO_FIT.
 *
 * Stage A, the seed: one correspondence pass per seed without a non-finite word.  The best seed has the largest count; ties go to the
 * smaller sum d2, then to the lower seed index.  (A seed with a non-finite word loses to every other.)
 * Stage B, refinement: `iterations` times from the best seed: pass, then solve; no convergence test.  A pass with fewer than min_pairs
 * accepted rows ends the pair with EPC_STATUS_NO_FIT.  (The first pass of stage B is the best seed's pass of stage A: the implementation
 * does it once.)
 * Final pass: one more correspondence pass under the result (with iterations == 0: under the best seed).  Fewer than min_pairs accepted
 * rows here is EPC_STATUS_NO_FIT too.
 *
 * Outputs -- the call writes every word of all four:
 *   pose (num_pairs, 12) float64: [R | t], source into target -- the last solve's, or the best seed's own words with iterations == 0.
 *   fit (num_pairs, 2) float64: sum d2 / m of the final pass (the mean squared residual, metres squared) and m / (source rows that are
 *       not absent), the overlap.
 *   info (num_pairs, 4) int32: the best seed, m of the final pass, the source rows and the target rows that are not absent.
 *   status (num_pairs) int32: 0, EPC_STATUS_NO_PAIR or EPC_STATUS_NO_FIT.
 * EPC_STATUS_NO_PAIR: an index of the pair lies outside [0, num_clouds) -- so the -1 entries of a revisit search pass straight through
 * -- or every seed of the pair holds a non-finite word.  A flagged pair (either bit) has a NaN pose (0x7ff8000000000000), a NaN fit, best
 * seed -1 and m 0; its row counts are those of its clouds, or 0 and 0 where an index is outside.
 *
 * Nothing is read back to the host and every grid is sized from the arguments alone, so the call is capturable in a graph and the
 * graph replays on other clouds, pairs and seeds.  No memset on `stream`; no kernel reads a workspace word that an earlier kernel of
 * the same call has not written (no atomics: there is nothing to clear).
 *
 * How: one launch counts the rows of every pair and checks its indices and seeds; a correspondence launch per pass -- grid (pair, seed,
 * chunk of 256 source rows), the target staged once per workgroup in LDS as three float arrays with +Inf in the absent rows, every lane
 * keeping one source row in registers and reading four targets per wave-uniform 16-byte LDS read, packed float32 arithmetic on two
 * targets at once, the chunk's 17 subtree sums written to the workspace -- and a solve launch behind each that finishes the tree,
 * chooses the seed or solves, and after the final pass writes the outputs: num_seeds' passes in one launch, then `iterations` of one
 * (2 * iterations + 3 launches).
 *
 * EPC_EINVAL, with nothing launched and nothing written, unless n % 32 == 0 and 32 <= n <= 4096, num_clouds >= 1, 0 <= num_pairs <= 2^20,
 * 1 <= num_seeds <= 64 (1 where seeds is NULL), max_dist is finite and > 0, 0 <= iterations <= 64, 3 <= min_pairs <= n, every pointer
 * but seeds is non-NULL, and clouds and the workspace are 16-byte aligned.  num_pairs == 0 returns EPC_OK with nothing launched.
 * EPC_ENOMEM for a workspace shorter than epcnet_pair_register_workspace_bytes(num_pairs, num_seeds, n), which launches nothing and
 * returns 0 for arguments the entry refuses.
 *
 * Not covered: global, feature-based registration from an unknown pose; point-to-plane metrics; robust kernels beyond the gate;
 * symmetric correspondences; the covariance of the estimate. */
size_t epcnet_pair_register_workspace_bytes(int num_pairs, int num_seeds, int n);
int epcnet_pair_register(const float* clouds, int num_clouds, int n, const int32_t* pairs, int num_pairs, const double* seeds, int num_seeds,
                         double max_dist, int iterations, int min_pairs, double* pose, double* fit, int32_t* info, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_PAIRS_H */
