/* tcfd_ns2d_adjoint.h -- the adjoint model of the fused spectral step: two entry points of libtcfd_hip.so next to those of
 * tcfd.h (same plans, same status codes, same conventions; ABI revision 13, no existing entry changed).
 *
 * A host that needs them includes this header after (or instead of) tcfd.h and looks the symbols up: a library built before
 * them loads, but lacks them.
 */
#ifndef TCFD_NS2D_ADJOINT_H
#define TCFD_NS2D_ADJOINT_H

#include "tcfd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What torch autograd derives from `steps` steps of the stepper when the state requires grad, in ONE call: the reverse of
 * tcfd_ns2d_step_imex with the same fa / beta / gdt / mu_num / mu_den / base0 (the same three may be NULL), from the saved INPUT
 * of every step -- nstages x steps intermediate states are never stored, they are recomputed.
 *   saved  (steps, batch, n, m) complex, read only: saved[s] = the state step s started from.  A host fills it by calling the
 *          forward once per step with w_in = saved[s], w_out = saved[s + 1] (the last result goes wherever the host wants it)
 *   g_out  (batch, n, m) complex, read only: cotangent of the last step's result
 *   g_in   (batch, n, m) complex: cotangent of saved[0]; g_out itself (in place) or disjoint from it, must not overlap saved
 *   pre    (n, m) real = mask / c,  post (4, n, m) complex = -(c / n^2) conj(a_f): the tables of tcfd_ns2d_explicit_terms_vjp /
 *          tcfd_ns2d_vjp_combine, on the device, in the plan's precision
 * Steps are reversed last first.  Per step the stage states u_0 = saved[s], u_1 .. u_{nstages-1} come from the forward code
 * (tcfd_ns2d_explicit_terms' sweep + the stage update) into the workspace; then, k = nstages - 1 .. 0, with r = 1 / (1 - mu_den[k] L):
 *     G = hbar + gdt[k] r ubar ,   fbar = fa[k] G ,   hbar <- beta[k] G ,   bbar = (1 + mu_num[k] L) r ubar
 *     ubar <- J_F(u_k)^T fbar + (base0[k] ? 0 : bbar) ,   ubar_start += base0[k] ? bbar : 0
 * (hbar = 0 at the last stage of every step; ubar_start joins ubar after stage 0).  The forcing is state-independent and does
 * not enter.  Per reversed stage: one element-wise launch, the launches of tcfd_ns2d_explicit_terms_vjp, one closing launch.
 * Workspace: tcfd_ns2d_step_vjp_workspace_bytes(plan, batch, nstages) = 12 + nstages chunk-sized fields, the chunk that of
 * tcfd_ns2d_step (tcfd_ns2d_plan_chunking): it stops growing at one chunk; 0 for an empty batch or nstages outside 1..32.
 * Samples are independent: a chunked call gives the bits of its samples run alone.  No atomics: two runs give the same bits.
 * TCFD_EINVAL (tcfd_last_error names the case): a NULL pointer, steps <= 0, nstages outside 1..32, g_in overlapping saved or
 * overlapping g_out without being g_out; a
 * workspace smaller than reported is TCFD_EWORKSPACE as for every call (tcfd.h, Conventions). */
size_t tcfd_ns2d_step_vjp_workspace_bytes(const tcfd_ns2d_plan* plan, long batch, int nstages);
int tcfd_ns2d_step_vjp(const tcfd_ns2d_plan* plan, const void* saved, const void* g_out, const void* pre, const void* post,
                       void* g_in, long batch, int nstages, const double* fa, const double* beta, const double* gdt,
                       const double* mu_num, const double* mu_den, const int* base0, int steps, void* workspace,
                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
