/* epcnet_forms.h -- test / tuning entries that name a kernel's form: the eighth header of libepcnet_hip.so.
 *
 * Same conventions, status codes and grammar as epcnet.h (plain C, caller-owned buffers, asynchronous on `stream`, EPC_OK or a negative
 * epc_status, epc_last_error() for the text); epc-net_amd/lib.py derives the binding of these entries from this file exactly as it
 * derives the others from the earlier headers.  The entries carry the prefix epcnet_: epcnet.h stays the complete list of the
 * library's epc_ symbols, and no product path calls what is declared here.
 */
#ifndef EPCNET_FORMS_H
#define EPCNET_FORMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ProxyConv block entry of epcnet.h -- same arguments, same checks -- with the form of the f32 kernel chosen by the caller:
 * form 0 = count, list and rows looked up pass by pass, 1 = a tile's counts and lists in one coalesced prologue and straight-line
 * passes where every list of the tile holds exactly 20 entries (what the entry of epcnet.h runs).  Both forms leave bit-identical out
 * and x_next (tests/test_gpu_block_feed.py).  The fp16 kernel (x16 != NULL) has one form and ignores the argument.  An explicit
 * argument, because the library reads no environment.  EPC_EINVAL for any other form. */
int epcnet_block_fwd_form(const float* x, const void* x16, const float* xyz, const void* idx, int idx_u16, const int32_t* cnt,
                          const float* kth, int cap, const void* packed_block, int has_next, int num_clouds, int n, int knn,
                          float* out, void* out16, int out_stride, int out_off, float* x_next, void* x_next16, int32_t* status,
                          int form, void* stream);

/* epc_conv5_assign_f32_fwd of epcnet.h -- same arguments, same checks -- with the form of the kernel chosen by the caller: form 0 = the
 * kernel with plain loads and stores and the epilogue's bf16 split value by value, 1 = the once-touched bytes (outputs, cat rows)
 * moved with the non-temporal hint and the epilogue's vector work trimmed (what the entry of epcnet.h and the pipeline launch).
 * Both forms leave bit-identical feat_frag, rnorm, assign, assign_frag and apart (tests/test_gpu_conv5_forms.py).  EPC_EINVAL for
 * any other form. */
int epcnet_conv5_assign_f32_fwd_form(const float* cat, int cin, const void* packed_conv5, int num_points_total, void* feat_frag,
                                     float* rnorm, float* assign, void* assign_frag, float* apart, int form, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPCNET_FORMS_H */
