/* tcfd_ns2d_bundle.h -- the tangent-linear model of the fused spectral step for a BUNDLE of K tangents per state: three entry
 * points of libtcfd_hip.so next to those of tcfd.h (same plans, same status codes, same conventions; ABI revision 13, no
 * existing entry changed).
 *
 * A host that needs them includes this header after (or instead of) tcfd.h and looks the symbols up: a library built before
 * them loads, but lacks them.
 */
#ifndef TCFD_NS2D_BUNDLE_H
#define TCFD_NS2D_BUNDLE_H

#include "tcfd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tcfd_ns2d_explicit_terms_jvp / tcfd_ns2d_step_jvp with `ntangents` perturbations of every state instead of one: what
 * ntangents calls on the same state compute (Lyapunov spectra and vectors, block Krylov, several Gauss-Newton directions), with
 * the state's share of the work -- its column passes, its four row transforms per row pair, its stage update -- done once.
 *   w / w_in, out_f, w_out   (batch, n, m) complex
 *   dw / dw_in, out_df, dw_out   (ntangents, batch, n, m) complex, contiguous: tangent k of field b is field k * batch + b
 * out_df[k] = F'(w) dw[k]; dw_out[k] = d(w_out)/d(w_in) . dw_in[k].  Member k has the bits of the bundle call with that member
 * alone (ntangents = 1), whatever the other members hold, and the state the bits it has with any other tangents; against
 * tcfd_ns2d_step_jvp on (w, dw[k]) member k agrees to rounding (1e-12 relative in complex128, 2e-5 in complex64), bit for bit
 * only where both run the same row kernels (complex128, n = 5 * 2^k).  out_f may be NULL.
 * Arguments and status codes as tcfd_ns2d_step_jvp (fa / mu_den / base0 may be NULL), and TCFD_EINVAL for ntangents outside
 * 1..65535, for a plan with per-sample parameters (tcfd_ns2d_plan_set_ensemble), and for arrays that overlap: an output of
 * explicit_terms_jvp_bundle may not overlap an input or the other output; in step_jvp_bundle no state array may overlap a tangent
 * array, and w_out (dw_out) is w_in (dw_in) itself -- in place -- or disjoint from it.
 * Workspace: tcfd_ns2d_bundle_workspace_bytes(plan, batch, ntangents), non-decreasing in batch and in ntangents (0 for an empty
 * batch or ntangents outside 1..65535); a smaller one is TCFD_EWORKSPACE (tcfd_last_error gives both numbers).  A call runs chunk
 * by chunk, and within a chunk tangent group by tangent group, sized so that the plane sets in flight fit the last-level cache.
 * Samples are independent: a chunked call gives the bits of its samples run alone.  No atomics: two runs give the same bits. */
size_t tcfd_ns2d_bundle_workspace_bytes(const tcfd_ns2d_plan* plan, long batch, int ntangents);
int tcfd_ns2d_explicit_terms_jvp_bundle(const tcfd_ns2d_plan* plan, const void* w, const void* dw, void* out_f, void* out_df,
                                        long batch, int ntangents, void* workspace, size_t workspace_bytes, void* stream);
int tcfd_ns2d_step_jvp_bundle(const tcfd_ns2d_plan* plan, const void* w_in, const void* dw_in, void* w_out, void* dw_out,
                              long batch, int ntangents, int nstages, const double* fa, const double* beta, const double* gdt,
                              const double* mu_num, const double* mu_den, const int* base0, int steps, void* workspace,
                              size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
