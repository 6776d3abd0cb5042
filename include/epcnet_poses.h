/* epcnet_poses.h -- relations and training tuples from the records' poses: the second header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from epcnet.h.  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the library's epc_
 * symbols, and this family -- float64 poses, integer draws, nothing of the network -- is declared on its own.
 */
#ifndef EPCNET_POSES_H
#define EPCNET_POSES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* Relations and training tuples from poses (generating_queries/generate_training_tuples_baseline.py:52-62,   */
/* generate_test_sets.py:95-104, utils/loading_pointclouds.py:102-168 get_query_tuple) -- csrc/pose_tuples.hip */
/* ------------------------------------------------------------------------------------------------------ */
/* Poses are (rows, 2) FLOAT64 in device memory, (northing, easting): a UTM northing near 5.7e6 has a float32 spacing of 0.5 m.
 * The squared distance of two poses is d2 = dx * dx + dy * dy in float64, every operation rounded once (no FMA): numpy's float64
 * decides every relation alike.  A radius travels as `const double* radius`: ONE double in HOST memory, read during the call.  "Within r" is
 * d2 <= r * r (inclusive, sklearn KDTree.query_radius); a NEGATIVE of a record lies strictly outside: d2 > r_neg * r_neg; a POSITIVE
 * of record i is a record c != i within r_pos.  A NaN coordinate makes its pose neither.
 *
 * epcnet_pose_radius_count: lens[q] = the number of database poses within r of query pose q (num_q int32).
 * epcnet_pose_radius_fill:  the same lens, and padded (num_q, width) int32: the indices of those poses in ascending order, the rest of
 * the row -2 -- the tables of retrieval.PackedTruth.  A row longer than `width` is truncated and ORs 1 into *status (one device
 * int32, sticky: the caller clears it).  num_db <= 2^24. */
int epcnet_pose_radius_count(const double* query, int num_q, const double* db, int num_db, const double* radius, int32_t* lens,
                             void* stream);
int epcnet_pose_radius_fill(const double* query, int num_q, const double* db, int num_db, const double* radius, int width, int32_t* lens,
                            int32_t* padded, int32_t* status, void* stream);
/* counts[i] = the number of positives of record i: records c != i within r_pos (num int32; num <= 2^24). */
int epcnet_pose_pos_count(const double* poses, int num, const double* r_pos, int32_t* counts, void* stream);

/* The draw.  Every selection below is "the k records of a set with the smallest 64-bit value (hash << 32) | id", where
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16          (uint32 arithmetic)
 *   s = mix((uint32)seed);  for w in ((uint32)(seed >> 32), (uint32)step, (uint32)(step >> 32), key, stream):  s = mix(s ^ w)
 *   hash(c) = mix(s ^ c)
 * for the record id c, the key's id, and the stream number of the selection.  The values are distinct (the id is part of them), so a
 * selection does not depend on the order in which threads meet the records: any implementation draws the same tuples
 * (tests/tuples_ref.py is the numpy restatement). */
#define EPC_TUPLE_STREAM_POSITIVES 0
#define EPC_TUPLE_STREAM_CANDIDATES 1
#define EPC_TUPLE_STREAM_NEGATIVES 2
#define EPC_TUPLE_STREAM_OTHER 3
/* status bits of a key's slot (ORed into status[b]: sticky, the caller clears them) */
#define EPC_TUPLE_FEW_POSITIVES 1 /* fewer than P positives: the missing slots are -1 (the reference's "FAULTY TUPLE")           */
#define EPC_TUPLE_FEW_NEGATIVES 2 /* fewer than Nn negatives: the missing slots are -1                                           */
#define EPC_TUPLE_NO_OTHER 4      /* no eligible other negative: -1 (the reference's "NO OTHER NEG")                             */
#define EPC_TUPLE_BAD_KEY 8       /* the key is outside [0, num): every slot -1, cand_count 0                                    */
#define EPC_TUPLE_MAX_CAND 4096
#define EPC_TUPLE_MAX_HARD 32
#define EPC_TUPLE_MAX_IDS 64
/* Phase A, per key keys[b] (num_keys int32 in device memory, read when the kernel runs): the min(C, #negatives) negatives of the key
 * with the smallest values of stream 1, written in ASCENDING ID order to cand[b][0 .. cand_count[b]) -- cand (num_keys, max_cand) and
 * cand_count (num_keys) are the buffers epc_mine_topk takes; entries behind the count are left alone.  It replaces "shuffle the
 * negatives, take the first 4000" (train.py:373-377).  status (num_keys int32) and flagged (num_keys int32, may be NULL: the last key
 * that set a bit in the slot) as in epcnet_tuple_sample.  One workgroup per key streams the poses; the selection's threshold comes from
 * radix passes over the 64-bit values with an LDS histogram; no storage proportional to num, no global atomics.
 * Preconditions (else EPC_EINVAL, nothing launched): 0 < num <= 2^24, 0 < max_cand <= EPC_TUPLE_MAX_CAND, 0 <= num_keys <= 65535. */
int epcnet_tuple_candidates(const double* poses, int num, const int32_t* keys, int num_keys, const double* r_neg, long long seed,
                            long long step, int max_cand, int32_t* cand, int32_t* cand_count, int32_t* status, int32_t* flagged,
                            void* stream);
/* Phase B, per key: ids[b] = { key, P positives, Nn negatives, the other negative } (num_keys, 1 + P + Nn + 1) int32 -- the order of
 * TrainStep.step_ids / train.py:252 -- by the rules of get_query_tuple:
 *   positives   the P positives of the key with the smallest values of stream 0, in that order;
 *   negatives   first the entries of hard[b][0 .. H) (device int32, may be NULL with H = 0; H <= EPC_TUPLE_MAX_HARD) that lie in
 *               [0, num), in the order given, an entry equal to an earlier one dropped, at most Nn of them (they are NOT tested
 *               against r_neg: the caller mined them from negatives); then the negatives of the key with the smallest values of
 *               stream 2 that are not among those, in that order, until there are Nn;
 *   other       eligible are the records of [0, num) that are a positive neither of the key nor of any chosen negative -- no record
 *               is its own positive, so the key itself and a chosen negative far from the other ones ARE eligible, as in the
 *               reference; of those the one with the smallest value of stream 3.
 * A slot that cannot be filled is -1 and sets EPC_TUPLE_FEW_POSITIVES / _FEW_NEGATIVES / _NO_OTHER in status[b] (ops.CloudBank turns
 * a -1 into a NaN loss and names the slot); a key outside [0, num) sets EPC_TUPLE_BAD_KEY and gets -1 in every slot.  flagged[b]
 * (may be NULL) receives the key whenever a bit is set.  One workgroup per key; the small selections rank at most 64 survivors of
 * the radix threshold in LDS.  Preconditions (else EPC_EINVAL): 0 < num <= 2^24, P >= 0, Nn >= 0, P + Nn + 2 <= EPC_TUPLE_MAX_IDS,
 * 0 <= H <= EPC_TUPLE_MAX_HARD, 0 <= num_keys <= 65535. */
int epcnet_tuple_sample(const double* poses, int num, const int32_t* keys, int num_keys, const double* r_pos, const double* r_neg,
                        long long seed, long long step, int num_pos, int num_neg, const int32_t* hard, int num_hard, int32_t* ids,
                        int32_t* status, int32_t* flagged, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_POSES_H */
