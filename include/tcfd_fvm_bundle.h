/* tcfd_fvm_bundle.h -- the tangent-linear finite-volume step for a BUNDLE of K tangents per state: one entry point of
 * libtcfd_hip.so next to those of tcfd.h (same plans, same status codes, same conventions; ABI revision 13, no existing entry
 * changed).
 *
 * A host that needs it includes this header after (or instead of) tcfd.h and looks the symbol up: a library built before it
 * loads, but lacks it.
 */
#ifndef TCFD_FVM_BUNDLE_H
#define TCFD_FVM_BUNDLE_H

#include "tcfd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest ntangents a plan takes: 1 + ntangents fields of one sample fit the launch grids' field dimension (65535) */
#define TCFD_FVM_MAX_TANGENTS 65534

/* Makes `plan` a BUNDLE plan of ntangents = K perturbations per state (1 .. TCFD_FVM_MAX_TANGENTS), or a plain plan again
 * (0): what K calls of a tangent plan (tcfd_fvm_plan_set_tangent) on the same state compute -- Lyapunov spectra and vectors,
 * block Krylov, several Gauss-Newton directions -- with the state's share of the work done once: its stencil loads, its
 * explicit terms, the state-only part of every flux tangent, its stage targets and its pressure projections.
 *
 * On a bundle plan tcfd_fvm_explicit_terms and tcfd_fvm_step take batch = (1 + K) B fields: fields [0, B) of every array are
 * the B states, fields [(1 + k) B, (2 + k) B) tangent k of each, k < K (K = 1: the pair layout of a tangent plan).
 *   explicit_terms   kx / ky fields [0, B) = F(u), fields of tangent k = J_F(u) du_k
 *   step             out fields [0, B) = the stepped states, fields of tangent k = d(u_out)/d(u_in) . du_k; steps == 0 copies all
 * The state has the bits of the plain plan's call, tangent k the bits of a tangent plan's call on (u, du_k), whatever the other
 * members hold; no atomics, so two runs give the same bits.  Workspace: tcfd_fvm_workspace_bytes(plan, (1 + K) B).
 * tcfd_fvm_project is linear per field and unchanged.
 *
 * With per-sample parameters (tcfd_fvm_plan_set_ensemble, count members) the plan takes batch == (1 + K) count; state b and all
 * its tangents run with member b's values.
 *
 * TCFD_EINVAL, named in tcfd_last_error and returned before any device call: a null plan; ntangents outside
 * 0 .. TCFD_FVM_MAX_TANGENTS; ntangents > 0 on a tangent plan (and tcfd_fvm_plan_set_tangent(plan, 1) on a bundle plan) -- the
 * two exclude each other, and the refused call leaves the plan as it was; and, from the calls on a bundle plan: a batch that is
 * no multiple of 1 + K, more than 65535 fields in all (the launch grids' field dimension), an ensemble batch other than
 * (1 + K) count, and tcfd_fvm_explicit_terms_vjp / tcfd_fvm_step_vjp (forward over reverse is not provided). */
int tcfd_fvm_plan_set_tangent_bundle(tcfd_fvm_plan* plan, int ntangents);

#ifdef __cplusplus
}
#endif
#endif
