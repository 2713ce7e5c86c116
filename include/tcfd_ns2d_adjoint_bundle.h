/* tcfd_ns2d_adjoint_bundle.h -- the adjoint model of the fused spectral step for a BUNDLE of K cotangents per trajectory: three
 * entry points of libtcfd_hip.so next to those of tcfd.h (same plans, same status codes, same conventions; ABI revision 13, no
 * existing entry changed).
 *
 * A host that needs them includes this header after (or instead of) tcfd.h and looks the symbols up: a library built before
 * them loads, but lacks them.
 */
#ifndef TCFD_NS2D_ADJOINT_BUNDLE_H
#define TCFD_NS2D_ADJOINT_BUNDLE_H

#include "tcfd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tcfd_ns2d_explicit_terms_vjp / tcfd_ns2d_step_vjp (tcfd_ns2d_adjoint.h) with `ncotangents` cotangents of every trajectory
 * instead of one: what ncotangents calls on the same saved states compute (singular vectors by block iteration on J^T J,
 * sensitivities of several observables, rows of a Jacobian, block Gauss-Newton), with the state's share of the work -- the
 * recomputation of the stage states, its opening column pass per reversed stage, its four row transforms per row pair -- done once.
 *   w                  (batch, n, m) complex;  saved  (steps, batch, n, m) complex, read only, as for tcfd_ns2d_step_vjp
 *   gm, g_out, g_in    (ncotangents, batch, n, m) complex, contiguous: cotangent k of field b is field k * batch + b
 *   xout               (ncotangents, 4, batch, n, m) complex: the four half spectra X_f of tcfd_ns2d_explicit_terms_vjp per cotangent
 *   pre, post          the tables of tcfd_ns2d_step_vjp
 * g_in[k] = (d result / d saved[0])^T g_out[k].  g_in is g_out itself (in place) or disjoint from it and does not overlap saved;
 * xout overlaps neither w nor gm.  Member k has the bits of the bundle call with that member alone (ncotangents = 1), whatever the
 * other members hold; against tcfd_ns2d_step_vjp on (saved, g_out[k]) member k agrees to rounding (1e-12 relative in complex128,
 * 2e-5 in complex64), bit for bit only where both run the same row kernel.
 * Arguments and status codes as tcfd_ns2d_step_vjp (fa / mu_den / base0 may be NULL), and TCFD_EINVAL (tcfd_last_error names the
 * case) for a NULL pointer, steps <= 0, nstages outside 1..32, ncotangents outside 1..65535, batch x ncotangents above the largest
 * batch of one call, a plan with per-sample parameters (tcfd_ns2d_plan_set_ensemble), and the overlaps above.
 * Workspace: tcfd_ns2d_step_vjp_bundle_workspace_bytes(plan, batch, ncotangents, nstages), non-decreasing in batch and in
 * ncotangents (0 for an empty batch, ncotangents outside 1..65535 or nstages outside 1..32); explicit_terms_vjp_bundle takes the
 * size of nstages = 1.  A smaller one is TCFD_EWORKSPACE with nothing touched (tcfd_last_error gives both numbers).  A call runs
 * chunk by chunk, and within a chunk cotangent group by cotangent group, sized as the tangent bundle's (tcfd_ns2d_bundle.h) so
 * that the plane sets in flight fit the last-level cache.  Samples are independent: a chunked call gives the bits of its samples
 * run alone.  No atomics: two runs give the same bits. */
size_t tcfd_ns2d_step_vjp_bundle_workspace_bytes(const tcfd_ns2d_plan* plan, long batch, int ncotangents, int nstages);
int tcfd_ns2d_explicit_terms_vjp_bundle(const tcfd_ns2d_plan* plan, const void* w, const void* gm, void* xout, long batch,
                                        int ncotangents, void* workspace, size_t workspace_bytes, void* stream);
int tcfd_ns2d_step_vjp_bundle(const tcfd_ns2d_plan* plan, const void* saved, const void* g_out, const void* pre, const void* post,
                              void* g_in, long batch, int ncotangents, int nstages, const double* fa, const double* beta,
                              const double* gdt, const double* mu_num, const double* mu_den, const int* base0, int steps,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
