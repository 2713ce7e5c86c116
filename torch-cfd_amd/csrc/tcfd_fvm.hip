// tcfd_fvm.hip -- MI355X (gfx950) kernels + C ABI of the finite-volume (staggered MAC grid) Navier-Stokes solver:
// explicit Runge-Kutta stages with a pressure projection after each (reference: torch_cfd/fvm.py
// NavierStokes2DFVMProjection :334 / RKStepper :196, pressure.py PressureProjection :68 / Pseudoinverse :153).
//
// Data layout: ux[b][i][j] sits at the x-face (i + 1, j + 1/2) of cell (i, j), uy[b][i][j] at the y-face (i + 1/2, j + 1);
// q (pressure increment) and the divergence at the cell centres.  Periodic in both axes, square n x n.
//
// Launch sequence of one RK stage i (every kernel instantiated for fp64 and fp32, chosen by the plan's dtype):
//   k_fvm_apply    u_i = u*_i - grad q_i (forward differences of q; skipped for stage 0, whose state is u0)
//   k_fvm_stage    k_i = explicit_terms(u_i) in registers; u*_m (+)= c_mi k_i for every later stage m and the final sum
//                  (one instantiation per advection scheme of the plan, chosen by a host-side switch at launch)
//   k_fvm_div      backward-difference divergence of the next u*
//   tcfd_rfft2 -> k_fvm_mul (x inverse eigenvalues) -> tcfd_irfft2: q of the next stage
// The transforms are the spectral solver's kernels (tcfd_ns2d.hip) on a table-free plan held by the FVM plan.
//
// Reverse of one step (tcfd_fvm_step_vjp; u_bar is the cotangent of the step's result, overwritten by that of its input):
//   stages 0 .. s-2 of the forward (k_fvm_stage + projection) rebuild the stage states u_1 .. u_{s-1} from the saved u0
//   projection of u_bar, its apply pass k_fvm_apply_adj: mu = P u_bar;  u_bar = mu;  kbar_j = b_j mu
//   for i = s-1 .. 0:  k_fvm_stage_vjp  g_i = J_F(u_i)^T kbar_i  (i = 0: added into u_bar; done)
//                      projection of g_i, k_fvm_apply_adj: mu_i = P g_i;  u_bar += mu_i;  kbar_j (+)= a_ij mu_i (j < i)
//
// Tangent-linear step (a plan with tcfd_fvm_plan_set_tangent on): every field array holds PAIRS, fields [0, B) the state and
// fields [B, 2 B) its perturbation.  k_fvm_stage_jvp replaces k_fvm_stage and runs over the B samples: it forms k = F(u) by the
// state kernel's own code and dk = J_F(u) du from the same stencil, and writes the RK targets of both halves.  Every other pass
// (k_fvm_div, the transforms, k_fvm_mul, k_fvm_apply) is linear per field and runs unchanged over the 2 B fields.
//
// Tangent bundle (a plan with tcfd_fvm_plan_set_tangent_bundle K, include/tcfd_fvm_bundle.h): every field array holds 1 + K fields
// per sample, fields [0, B) the state and fields [(1 + k) B, (2 + k) B) perturbation k.  k_fvm_stage_jvp_bundle replaces
// k_fvm_stage and runs over the B samples: the state's loads, explicit terms and the state-only share of every flux tangent once,
// then the K members by k_fvm_stage_jvp's arithmetic (member k has the bits of a tangent plan on (u, du_k)).  Every other pass
// runs unchanged over the (1 + K) B fields.
//
// Ensemble plan (tcfd_fvm_plan_set_ensemble): sample b of a call runs with its own viscosity, drag and forcing amplitude.  The
// stage kernels (k_fvm_stage, k_fvm_stage_jvp, k_fvm_stage_jvp_bundle, k_fvm_stage_vjp) have an EnsConst instantiation that reads
// the three values of member blockIdx.z from a plan-owned table; every other pass reads no physics and runs unchanged.
//
// Every arithmetic expression restates the reference's operation order; floating-point contraction is off in this file
// so that a * b + c rounds twice as the reference's tensor ops do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tcfd_host.hpp"
#include "../../include/tcfd_fvm_bundle.h"

#pragma clang fp contract(off)

namespace {

// per-point scalars, converted to the field type once (the reference multiplies fp32 tensors by Python floats, which
// torch rounds to fp32 first)
template <typename T>
struct StageConst {
    T cfl;       // dt / h                (Courant number = cfl * u)
    T inv_h2;    // 1 / h**2              (laplacian scale per axis)
    T sum_s;     // 1 / h**2 + 1 / h**2   (sum(scales))
    T nu;        // viscosity / density
    T neg_drag;  // -drag
    T h;
    int drag_on;
};

// Per-sample physics (tcfd_fvm_plan_set_ensemble): the constants of ONE member of an ensemble plan.  The plan owns a device table
// of count x {nu / density, -drag, forcing_scale} in the field type; a workgroup belongs to one sample (blockIdx.z), so the three
// values are workgroup-uniform loads and nothing is loaded per lane.  The device functions below are templates on the type of
// their constants, S: StageConst<T> is the scalar plan's and compiles to the code it always did, MemberConst<T> the ensemble's.
template <typename T>
struct MemberConst : StageConst<T> {
    T fscale;   // the member's forcing is fl(fscale * f), then added where f is added (1: today's sum)
};
template <typename S>
constexpr bool kScaledForcing = false;
template <typename T>
constexpr bool kScaledForcing<MemberConst<T>> = true;

constexpr int ENS_ROW = 3;   // values per member in the table

// The stage kernels are templates on the type S of their constants ARGUMENT.  S = StageConst<T> is the scalar plan's kernel: its
// argument list is what it was before per-sample physics existed, and so are the registers, scratch and occupancy of all 24
// instantiations (profiles/fvm_ensemble_kernel_resource_usage.txt).  S = EnsConst<T> is the ensemble plan's: the plan's
// constants and its member table, of which sample blockIdx.z reads row blockIdx.z.  The choice is made at compile time
// (if constexpr (kEnsemble<S>)); no kernel branches on a table at run time.  Keep the kernel bodies in the __global__
// functions: moving them into a shared inlined function changed the scalar kernels' register allocation (same file).
template <typename T>
struct EnsConst {
    StageConst<T> plan;
    const T* rows;   // ENS_ROW values per member; row 0 belongs to sample 0 of the launch
};
template <typename S>
constexpr bool kEnsemble = false;
template <typename T>
constexpr bool kEnsemble<EnsConst<T>> = true;

// the constants of member `b`: the plan's, with the member's nu, -drag and forcing scale.  drag_on is per member; -drag is
// exact in the field type up to underflow, where a drag that rounds to zero adds a zero.
template <typename T>
__device__ __forceinline__ MemberConst<T> member_const(const StageConst<T>& s, const T* __restrict__ ens, unsigned b) {
    const T* m = ens + (size_t)ENS_ROW * b;
    MemberConst<T> r;
    r.cfl = s.cfl;
    r.inv_h2 = s.inv_h2;
    r.sum_s = s.sum_s;
    r.h = s.h;
    r.nu = m[0];
    r.neg_drag = m[1];
    r.drag_on = m[1] < T(0);
    r.fscale = m[2];
    return r;
}

constexpr int MAXT = 4;   // stages of an explicit tableau (and so RK targets of one stage: the later stages + the final sum)

template <typename T>
struct Targets {
    T* x[MAXT];
    T* y[MAXT];
    T c[MAXT];
    int mode[MAXT];   // 1: P = u0 + c k,  2: P = P + c k,  3: P = u0
    int count;
};

__device__ __forceinline__ int wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// flux of the transported component c across the upper face of its control volume along one axis:
// apply_tvd_limiter(lax_wendroff, van_leer_limiter) of c interpolated with face velocity w, times w
// (interpolation.py:171 upwind, :246 lax_wendroff, :240 safe_div, :246 van_leer_limiter, :251 tvd; fvm.py:40 c * u)
template <typename T>
__device__ __forceinline__ T tvd_flux(T cm, T c0, T c1, T c2, T w, T cfl) {
    const bool pos = w > T(0);
    const T clow = pos ? c0 : c1;
    const T cr = cfl * w;
    const T d = c1 - c0;
    const T hp = c0 + (T(0.5) * (T(1) - cr)) * d;
    const T hn = c1 - (T(0.5) * (T(1) + cr)) * d;
    const T chigh = pos ? hp : hn;
    const T dd = d != T(0) ? d : T(1);
    const T r = pos ? (c0 - cm) / dd : (c2 - c1) / dd;
    const T rp1 = T(1) + r;
    const T phi = r > T(0) ? (T(2) * r) / (rp1 != T(0) ? rp1 : T(1)) : T(0);
    const T ci = clow - (clow - chigh) * phi;
    return ci * w;
}

// linear interpolation to the half-way point: floor_weight * shift(0) + ceil_weight * shift(1) (interpolation.py:16)
template <typename T>
__device__ __forceinline__ T half(T a, T b) { return T(0.5) * a + T(0.5) * b; }

// advection scheme of a plan (tcfd.h TCFD_FVM_*): the interpolation of the transported component to a face, a compile-time
// choice of the stage kernel and of its adjoint.  VAN_LEER reads the four cells cm .. c2 around the face (tvd_flux); the other
// three read the two cells c0, c1 next to it (face_flux), so their instantiations never form the +-2 neighbours' addresses.
constexpr int VAN_LEER = TCFD_FVM_VAN_LEER, UPWIND = TCFD_FVM_UPWIND, LINEAR = TCFD_FVM_LINEAR,
              LAX_WENDROFF = TCFD_FVM_LAX_WENDROFF;

// flux of the two-cell schemes across the face between c0 and c1, face velocity w:
//   UPWIND        where(w > 0, c0, c1) * w                                        (interpolation.py:102; w == 0 takes c1)
//   LINEAR        (0.5 c0 + 0.5 c1) * w                                           (:39, floor and ceil weights at offset 1/2)
//   LAX_WENDROFF  where(w > 0, c0 + 0.5 (1 - cr) d, c1 - 0.5 (1 + cr) d) * w      (:171; cr = cfl w, d = c1 - c0)
template <int SCHEME, typename T>
__device__ __forceinline__ T face_flux(T c0, T c1, T w, T cfl) {
    static_assert(SCHEME == UPWIND || SCHEME == LINEAR || SCHEME == LAX_WENDROFF, "two-cell schemes only");
    if constexpr (SCHEME == UPWIND) {
        return (w > T(0) ? c0 : c1) * w;
    } else if constexpr (SCHEME == LINEAR) {
        return half(c0, c1) * w;
    } else {
        const T cr = cfl * w;
        const T d = c1 - c0;
        const T hp = c0 + (T(0.5) * (T(1) - cr)) * d;
        const T hn = c1 - (T(0.5) * (T(1) + cr)) * d;
        return (w > T(0) ? hp : hn) * w;
    }
}

// the values both kinds of scheme share: the 5-point stencils of the two components around cell (i, j)
template <typename T>
struct Near {
    T x00, xm1, xp1, xjm1, xjp1, y00, ym1, yp1, yjm1, yjp1;
};

// ((convect + nu lap) + f) + (-drag) u from the advection terms of cell (i, j) (fvm.py:397-409)
template <typename T, typename S>
__device__ __forceinline__ void finish_point(const Near<T>& v, T adv_x, T adv_y, const T* __restrict__ fx,
                                             const T* __restrict__ fy, int i, int j, int n, const S& s, T& kx, T& ky) {
    // laplacian (finite_differences.py:150): (-2 u) * sum(scales) + (u[-1] + u[+1]) * s0 + (u[-1] + u[+1]) * s1
    T lap_x = (T(-2) * v.x00) * s.sum_s;
    lap_x = lap_x + (v.xm1 + v.xp1) * s.inv_h2;
    lap_x = lap_x + (v.xjm1 + v.xjp1) * s.inv_h2;
    T lap_y = (T(-2) * v.y00) * s.sum_s;
    lap_y = lap_y + (v.ym1 + v.yp1) * s.inv_h2;
    lap_y = lap_y + (v.yjm1 + v.yjp1) * s.inv_h2;

    kx = adv_x + s.nu * lap_x;
    ky = adv_y + s.nu * lap_y;
    if (fx) {
        const size_t p = (size_t)i * n + j;
        if constexpr (kScaledForcing<S>) {
            kx = kx + s.fscale * fx[p];
            ky = ky + s.fscale * fy[p];
        } else {
            kx = kx + fx[p];
            ky = ky + fy[p];
        }
    }
    if (s.drag_on) {
        kx = kx + v.x00 * s.neg_drag;
        ky = ky + v.y00 * s.neg_drag;
    }
}

// explicit_terms of both velocity components at cell (i, j) of field plane X / Y, the advection by the scheme SCHEME.
// VAN_LEER reads the -2 .. +2 stencils of both components and two corners, 20 loads; the two-cell schemes the 5-point
// stencils and the same corners, 12 loads: their branch never forms the +-2 indices.
template <int SCHEME, typename T, typename S>
__device__ __forceinline__ void explicit_point(const T* __restrict__ X, const T* __restrict__ Y, const T* __restrict__ fx,
                                               const T* __restrict__ fy, int i, int j, int n, const S& s,
                                               T& kx, T& ky) {
    auto at = [n](const T* p, int a, int b) { return p[(size_t)a * n + b]; };
    if constexpr (SCHEME == VAN_LEER) {
        const int im2 = wrap(i - 2, n), im1 = wrap(i - 1, n), ip1 = wrap(i + 1, n), ip2 = wrap(i + 2, n);
        const int jm2 = wrap(j - 2, n), jm1 = wrap(j - 1, n), jp1 = wrap(j + 1, n), jp2 = wrap(j + 2, n);

        // ---- ux: control volume centred at its own face, faces at (i + 3/2, j + 1/2) and (i + 1, j + 1)
        const T x00 = at(X, i, j);
        const T xm2 = at(X, im2, j), xm1 = at(X, im1, j), xp1 = at(X, ip1, j), xp2 = at(X, ip2, j);
        const T xjm2 = at(X, i, jm2), xjm1 = at(X, i, jm1), xjp1 = at(X, i, jp1), xjp2 = at(X, i, jp2);
        const T y00 = at(Y, i, j);
        const T yp1 = at(Y, ip1, j), yjm1 = at(Y, i, jm1), yp1jm1 = at(Y, ip1, jm1);
        T adv_x;
        {
            const T f_hi = tvd_flux(xm1, x00, xp1, xp2, half(x00, xp1), s.cfl);
            const T f_lo = tvd_flux(xm2, xm1, x00, xp1, half(xm1, x00), s.cfl);
            const T g_hi = tvd_flux(xjm1, x00, xjp1, xjp2, half(y00, yp1), s.cfl);
            const T g_lo = tvd_flux(xjm2, xjm1, x00, xjp1, half(yjm1, yp1jm1), s.cfl);
            adv_x = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
        // ---- uy: faces at (i + 1, j + 1) and (i + 1/2, j + 3/2)
        const T ym2 = at(Y, im2, j), ym1 = at(Y, im1, j), yp2 = at(Y, ip2, j);
        const T yjm2 = at(Y, i, jm2), yjp1 = at(Y, i, jp1), yjp2 = at(Y, i, jp2);
        const T xm1jp1 = at(X, im1, jp1);
        T adv_y;
        {
            const T f_hi = tvd_flux(ym1, y00, yp1, yp2, half(x00, xjp1), s.cfl);
            const T f_lo = tvd_flux(ym2, ym1, y00, yp1, half(xm1, xm1jp1), s.cfl);
            const T g_hi = tvd_flux(yjm1, y00, yjp1, yjp2, half(y00, yjp1), s.cfl);
            const T g_lo = tvd_flux(yjm2, yjm1, y00, yjp1, half(yjm1, y00), s.cfl);
            adv_y = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
        finish_point(Near<T>{x00, xm1, xp1, xjm1, xjp1, y00, ym1, yp1, yjm1, yjp1}, adv_x, adv_y, fx, fy, i, j, n, s, kx, ky);
    } else {
        const int im1 = wrap(i - 1, n), ip1 = wrap(i + 1, n);
        const int jm1 = wrap(j - 1, n), jp1 = wrap(j + 1, n);
        const T x00 = at(X, i, j);
        const T xm1 = at(X, im1, j), xp1 = at(X, ip1, j), xjm1 = at(X, i, jm1), xjp1 = at(X, i, jp1);
        const T y00 = at(Y, i, j);
        const T ym1 = at(Y, im1, j), yp1 = at(Y, ip1, j), yjm1 = at(Y, i, jm1), yjp1 = at(Y, i, jp1);
        const T yp1jm1 = at(Y, ip1, jm1), xm1jp1 = at(X, im1, jp1);   // the far ends of the lower faces' velocities
        T adv_x, adv_y;
        {   // ux: the faces of the van Leer branch, each flux from the two cells next to the face
            const T f_hi = face_flux<SCHEME>(x00, xp1, half(x00, xp1), s.cfl);
            const T f_lo = face_flux<SCHEME>(xm1, x00, half(xm1, x00), s.cfl);
            const T g_hi = face_flux<SCHEME>(x00, xjp1, half(y00, yp1), s.cfl);
            const T g_lo = face_flux<SCHEME>(xjm1, x00, half(yjm1, yp1jm1), s.cfl);
            adv_x = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
        {   // uy
            const T f_hi = face_flux<SCHEME>(y00, yp1, half(x00, xjp1), s.cfl);
            const T f_lo = face_flux<SCHEME>(ym1, y00, half(xm1, xm1jp1), s.cfl);
            const T g_hi = face_flux<SCHEME>(y00, yjp1, half(y00, yjp1), s.cfl);
            const T g_lo = face_flux<SCHEME>(yjm1, y00, half(yjm1, y00), s.cfl);
            adv_y = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
        finish_point(Near<T>{x00, xm1, xp1, xjm1, xjp1, y00, ym1, yp1, yjm1, yjp1}, adv_x, adv_y, fx, fy, i, j, n, s, kx, ky);
    }
}

// one thread per cell; blockIdx.z = sample
template <int SCHEME, typename T, typename S>
__global__ void __launch_bounds__(256) k_fvm_stage(const T* __restrict__ ux, const T* __restrict__ uy, const T* __restrict__ u0x,
                                                   const T* __restrict__ u0y, const T* __restrict__ fx, const T* __restrict__ fy,
                                                   T* __restrict__ kx_out, T* __restrict__ ky_out, Targets<T> tg, S s, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t plane = (size_t)n * n;
    const size_t base = (size_t)blockIdx.z * plane;
    T kx, ky;
    if constexpr (kEnsemble<S>)
        explicit_point<SCHEME>(ux + base, uy + base, fx, fy, i, j, n, member_const(s.plan, s.rows, blockIdx.z), kx, ky);
    else
        explicit_point<SCHEME>(ux + base, uy + base, fx, fy, i, j, n, s, kx, ky);
    const size_t p = base + (size_t)i * n + j;
    if (kx_out) {
        kx_out[p] = kx;
        ky_out[p] = ky;
    }
    for (int t = 0; t < tg.count; ++t) {
        const int mode = tg.mode[t];
        const T c = tg.c[t];
        T px, py;
        if (mode == 2) {
            px = tg.x[t][p];
            py = tg.y[t][p];
        } else {
            px = u0x[p];
            py = u0y[p];
        }
        if (mode != 3) {
            px = px + kx * c;
            py = py + ky * c;
        }
        tg.x[t][p] = px;
        tg.y[t][p] = py;
    }
}

// ---------------------------------------------------------------- tangent (Jacobian-vector products)
// Tangent of tvd_flux along (dcm, dc0, dc1, dc2, dw), by the branches torch's forward mode takes through the reference's ops,
// the conventions of tvd_flux_vjp below: the selections w > 0 and r > 0 carry no tangent, w enters through the Courant number
// and the final product ci * w, and the constant denominator 1 of safe_div (d == 0; 1 + r == 0 lies in the arm r > 0 never
// selects) has zero tangent.  Every term is a product of one tangent with state values, so the result is linear in the tangent
// bit for bit under a scaling by a power of two, and exactly zero for a zero tangent.
template <typename T>
__device__ __forceinline__ T tvd_flux_jvp(T cm, T c0, T c1, T c2, T w, T dcm, T dc0, T dc1, T dc2, T dw, T cfl) {
    const bool pos = w > T(0);
    const T clow = pos ? c0 : c1;
    const T dclow = pos ? dc0 : dc1;
    const T cr = cfl * w;
    const T d = c1 - c0;
    const T dd = dc1 - dc0;
    const T alpha = T(0.5) * (T(1) - cr);   // hp = c0 + alpha d
    const T beta = T(0.5) * (T(1) + cr);    // hn = c1 - beta d
    const T chigh = pos ? c0 + alpha * d : c1 - beta * d;
    // d chigh / d w = -cfl d / 2 in both branches
    const T dchigh = (pos ? dc0 + alpha * dd : dc1 - beta * dd) - (T(0.5) * (cfl * dw)) * d;
    const bool dnz = d != T(0);
    const T den = dnz ? d : T(1);
    const T dden = dnz ? dd : T(0);
    const T r = (pos ? c0 - cm : c2 - c1) / den;
    const T dr = ((pos ? dc0 - dcm : dc2 - dc1) - r * dden) / den;
    const bool lim = r > T(0);
    const T rp1 = T(1) + r;
    const T phi = lim ? (T(2) * r) / rp1 : T(0);
    const T dphi = lim ? (T(2) * dr - phi * dr) / rp1 : T(0);
    const T ci = clow - (clow - chigh) * phi;
    const T dci = dclow - ((dclow - dchigh) * phi + (clow - chigh) * dphi);
    return dci * w + ci * dw;
}

// tangent of face_flux along (dc0, dc1, dw), by the same rules
template <int SCHEME, typename T>
__device__ __forceinline__ T face_flux_jvp(T c0, T c1, T w, T dc0, T dc1, T dw, T cfl) {
    static_assert(SCHEME == UPWIND || SCHEME == LINEAR || SCHEME == LAX_WENDROFF, "two-cell schemes only");
    if constexpr (SCHEME == UPWIND) {
        const bool pos = w > T(0);
        return (pos ? dc0 : dc1) * w + (pos ? c0 : c1) * dw;
    } else if constexpr (SCHEME == LINEAR) {
        return half(dc0, dc1) * w + half(c0, c1) * dw;
    } else {
        const bool pos = w > T(0);
        const T cr = cfl * w;
        const T d = c1 - c0;
        const T dd = dc1 - dc0;
        const T alpha = T(0.5) * (T(1) - cr);
        const T beta = T(0.5) * (T(1) + cr);
        const T ci = pos ? c0 + alpha * d : c1 - beta * d;
        const T dci = (pos ? dc0 + alpha * dd : dc1 - beta * dd) - (T(0.5) * (cfl * dw)) * d;
        return dci * w + ci * dw;
    }
}

// (dkx, dky) = J (DX, DY) of explicit_point at cell (i, j): X / Y the state, DX / DY its perturbation.  The faces, their
// arguments and the order of the sums are explicit_point's, each flux replaced by its tangent; the Laplacian and the drag act on
// the perturbation, and the forcing, which does not depend on the state, drops out.  The state loads repeat the addresses
// explicit_point reads, so next to it in one kernel they are loaded once.  As there, the two-cell schemes never form the +-2
// addresses, of X and Y or of DX and DY.
template <int SCHEME, typename T, typename S>
__device__ __forceinline__ void explicit_point_jvp(const T* __restrict__ X, const T* __restrict__ Y, const T* __restrict__ DX,
                                                   const T* __restrict__ DY, int i, int j, int n, const S& s, T& dkx,
                                                   T& dky) {
    auto at = [n](const T* p, int a, int b) { return p[(size_t)a * n + b]; };
    const int im1 = wrap(i - 1, n), ip1 = wrap(i + 1, n);
    const int jm1 = wrap(j - 1, n), jp1 = wrap(j + 1, n);
    const T x00 = at(X, i, j), xm1 = at(X, im1, j), xp1 = at(X, ip1, j), xjm1 = at(X, i, jm1), xjp1 = at(X, i, jp1);
    const T y00 = at(Y, i, j), ym1 = at(Y, im1, j), yp1 = at(Y, ip1, j), yjm1 = at(Y, i, jm1), yjp1 = at(Y, i, jp1);
    const T yp1jm1 = at(Y, ip1, jm1), xm1jp1 = at(X, im1, jp1);
    const T dx00 = at(DX, i, j), dxm1 = at(DX, im1, j), dxp1 = at(DX, ip1, j), dxjm1 = at(DX, i, jm1), dxjp1 = at(DX, i, jp1);
    const T dy00 = at(DY, i, j), dym1 = at(DY, im1, j), dyp1 = at(DY, ip1, j), dyjm1 = at(DY, i, jm1), dyjp1 = at(DY, i, jp1);
    const T dyp1jm1 = at(DY, ip1, jm1), dxm1jp1 = at(DX, im1, jp1);
    T dadv_x, dadv_y;
    if constexpr (SCHEME == VAN_LEER) {
        const int im2 = wrap(i - 2, n), ip2 = wrap(i + 2, n), jm2 = wrap(j - 2, n), jp2 = wrap(j + 2, n);
        const T xm2 = at(X, im2, j), xp2 = at(X, ip2, j), xjm2 = at(X, i, jm2), xjp2 = at(X, i, jp2);
        const T ym2 = at(Y, im2, j), yp2 = at(Y, ip2, j), yjm2 = at(Y, i, jm2), yjp2 = at(Y, i, jp2);
        const T dxm2 = at(DX, im2, j), dxp2 = at(DX, ip2, j), dxjm2 = at(DX, i, jm2), dxjp2 = at(DX, i, jp2);
        const T dym2 = at(DY, im2, j), dyp2 = at(DY, ip2, j), dyjm2 = at(DY, i, jm2), dyjp2 = at(DY, i, jp2);
        {
            const T f_hi = tvd_flux_jvp(xm1, x00, xp1, xp2, half(x00, xp1), dxm1, dx00, dxp1, dxp2, half(dx00, dxp1), s.cfl);
            const T f_lo = tvd_flux_jvp(xm2, xm1, x00, xp1, half(xm1, x00), dxm2, dxm1, dx00, dxp1, half(dxm1, dx00), s.cfl);
            const T g_hi = tvd_flux_jvp(xjm1, x00, xjp1, xjp2, half(y00, yp1), dxjm1, dx00, dxjp1, dxjp2, half(dy00, dyp1), s.cfl);
            const T g_lo = tvd_flux_jvp(xjm2, xjm1, x00, xjp1, half(yjm1, yp1jm1), dxjm2, dxjm1, dx00, dxjp1,
                                        half(dyjm1, dyp1jm1), s.cfl);
            dadv_x = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
        {
            const T f_hi = tvd_flux_jvp(ym1, y00, yp1, yp2, half(x00, xjp1), dym1, dy00, dyp1, dyp2, half(dx00, dxjp1), s.cfl);
            const T f_lo = tvd_flux_jvp(ym2, ym1, y00, yp1, half(xm1, xm1jp1), dym2, dym1, dy00, dyp1, half(dxm1, dxm1jp1),
                                        s.cfl);
            const T g_hi = tvd_flux_jvp(yjm1, y00, yjp1, yjp2, half(y00, yjp1), dyjm1, dy00, dyjp1, dyjp2, half(dy00, dyjp1), s.cfl);
            const T g_lo = tvd_flux_jvp(yjm2, yjm1, y00, yjp1, half(yjm1, y00), dyjm2, dyjm1, dy00, dyjp1, half(dyjm1, dy00), s.cfl);
            dadv_y = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
    } else {
        {
            const T f_hi = face_flux_jvp<SCHEME>(x00, xp1, half(x00, xp1), dx00, dxp1, half(dx00, dxp1), s.cfl);
            const T f_lo = face_flux_jvp<SCHEME>(xm1, x00, half(xm1, x00), dxm1, dx00, half(dxm1, dx00), s.cfl);
            const T g_hi = face_flux_jvp<SCHEME>(x00, xjp1, half(y00, yp1), dx00, dxjp1, half(dy00, dyp1), s.cfl);
            const T g_lo = face_flux_jvp<SCHEME>(xjm1, x00, half(yjm1, yp1jm1), dxjm1, dx00, half(dyjm1, dyp1jm1), s.cfl);
            dadv_x = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
        {
            const T f_hi = face_flux_jvp<SCHEME>(y00, yp1, half(x00, xjp1), dy00, dyp1, half(dx00, dxjp1), s.cfl);
            const T f_lo = face_flux_jvp<SCHEME>(ym1, y00, half(xm1, xm1jp1), dym1, dy00, half(dxm1, dxm1jp1), s.cfl);
            const T g_hi = face_flux_jvp<SCHEME>(y00, yjp1, half(y00, yjp1), dy00, dyjp1, half(dy00, dyjp1), s.cfl);
            const T g_lo = face_flux_jvp<SCHEME>(yjm1, y00, half(yjm1, y00), dyjm1, dy00, half(dyjm1, dy00), s.cfl);
            dadv_y = -((f_hi - f_lo) / s.h + (g_hi - g_lo) / s.h);
        }
    }
    // finish_point on the perturbation, without the forcing
    finish_point(Near<T>{dx00, dxm1, dxp1, dxjm1, dxjp1, dy00, dym1, dyp1, dyjm1, dyjp1}, dadv_x, dadv_y, (const T*)nullptr,
                 (const T*)nullptr, i, j, n, s, dkx, dky);
}

// k_fvm_stage on a pair: fields [0, B) of every array the state, fields [B, 2 B) the perturbation, `pair` = B n^2 elements
// apart.  One thread per cell of the B samples; blockIdx.z = sample.  The state half is k_fvm_stage's own code (explicit_point,
// the same target expressions), so it is bit-equal to the plain kernel; the tangent half writes (du0, dk) to the same targets
// with the same modes and weights.
template <int SCHEME, typename T, typename S>
__global__ void __launch_bounds__(256) k_fvm_stage_jvp(const T* __restrict__ ux, const T* __restrict__ uy, const T* __restrict__ u0x,
                                                       const T* __restrict__ u0y, const T* __restrict__ fx, const T* __restrict__ fy,
                                                       T* __restrict__ kx_out, T* __restrict__ ky_out, Targets<T> tg, S s, int n,
                                                       size_t pair) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t plane = (size_t)n * n;
    const size_t base = (size_t)blockIdx.z * plane;
    T kx, ky, dkx, dky;
    if constexpr (kEnsemble<S>) {   // the state field b and its perturbation, field B + b, both step with member b = blockIdx.z
        const MemberConst<T> m = member_const(s.plan, s.rows, blockIdx.z);
        explicit_point<SCHEME>(ux + base, uy + base, fx, fy, i, j, n, m, kx, ky);
        explicit_point_jvp<SCHEME>(ux + base, uy + base, ux + pair + base, uy + pair + base, i, j, n, m, dkx, dky);
    } else {
        explicit_point<SCHEME>(ux + base, uy + base, fx, fy, i, j, n, s, kx, ky);
        explicit_point_jvp<SCHEME>(ux + base, uy + base, ux + pair + base, uy + pair + base, i, j, n, s, dkx, dky);
    }
    const size_t p = base + (size_t)i * n + j;
    const size_t dp = pair + p;
    if (kx_out) {
        kx_out[p] = kx;
        ky_out[p] = ky;
        kx_out[dp] = dkx;
        ky_out[dp] = dky;
    }
    for (int t = 0; t < tg.count; ++t) {
        const int mode = tg.mode[t];
        const T c = tg.c[t];
        T px, py, dpx, dpy;
        if (mode == 2) {
            px = tg.x[t][p];
            py = tg.y[t][p];
            dpx = tg.x[t][dp];
            dpy = tg.y[t][dp];
        } else {
            px = u0x[p];
            py = u0y[p];
            dpx = u0x[dp];
            dpy = u0y[dp];
        }
        if (mode != 3) {
            px = px + kx * c;
            py = py + ky * c;
            dpx = dpx + dkx * c;
            dpy = dpy + dky * c;
        }
        tg.x[t][p] = px;
        tg.y[t][p] = py;
        tg.x[t][dp] = dpx;
        tg.y[t][dp] = dpy;
    }
}

// ---------------------------------------------------------------- tangent bundle: K perturbations of one state
// What tvd_flux_jvp / face_flux_jvp compute from the state alone, kept per face while the members of a bundle pass: the same
// expressions in the same order, so a member's flux tangent has the bits of the pair kernel's.  UPWIND keeps the selected cell in
// `ci`, LINEAR the interpolated one; the fields a scheme does not read are never formed.
template <typename T>
struct FaceState {
    T w, d, ab, den, r, phi, cmh, ci;   // ab: alpha (w > 0) or beta;  cmh: clow - chigh
    bool pos, dnz, lim;
};

template <int SCHEME, typename T>
__device__ __forceinline__ FaceState<T> face_state(T cm, T c0, T c1, T c2, T w, T cfl) {
    FaceState<T> f{};
    f.w = w;
    if constexpr (SCHEME == LINEAR) {
        f.ci = half(c0, c1);
    } else if constexpr (SCHEME == UPWIND) {
        f.pos = w > T(0);
        f.ci = f.pos ? c0 : c1;
    } else {
        f.pos = w > T(0);
        const T cr = cfl * w;
        f.d = c1 - c0;
        const T alpha = T(0.5) * (T(1) - cr);
        const T beta = T(0.5) * (T(1) + cr);
        f.ab = f.pos ? alpha : beta;
        const T chigh = f.pos ? c0 + alpha * f.d : c1 - beta * f.d;
        if constexpr (SCHEME == LAX_WENDROFF) {
            f.ci = chigh;
        } else {
            const T clow = f.pos ? c0 : c1;
            f.dnz = f.d != T(0);
            f.den = f.dnz ? f.d : T(1);
            f.r = (f.pos ? c0 - cm : c2 - c1) / f.den;
            f.lim = f.r > T(0);
            const T rp1 = T(1) + f.r;
            f.phi = f.lim ? (T(2) * f.r) / rp1 : T(0);
            f.cmh = clow - chigh;
            f.ci = clow - f.cmh * f.phi;
        }
    }
    return f;
}

// the tangent of the face's flux along (dcm, dc0, dc1, dc2, dw): tvd_flux_jvp / face_flux_jvp with the state's share read from f
template <int SCHEME, typename T>
__device__ __forceinline__ T face_state_jvp(const FaceState<T>& f, T dcm, T dc0, T dc1, T dc2, T dw, T cfl) {
    if constexpr (SCHEME == LINEAR) {
        return half(dc0, dc1) * f.w + f.ci * dw;
    } else if constexpr (SCHEME == UPWIND) {
        return (f.pos ? dc0 : dc1) * f.w + f.ci * dw;
    } else {
        const T dd = dc1 - dc0;
        const T dchigh = (f.pos ? dc0 + f.ab * dd : dc1 - f.ab * dd) - (T(0.5) * (cfl * dw)) * f.d;
        if constexpr (SCHEME == LAX_WENDROFF) {
            return dchigh * f.w + f.ci * dw;
        } else {
            const T dclow = f.pos ? dc0 : dc1;
            const T dden = f.dnz ? dd : T(0);
            const T dr = ((f.pos ? dc0 - dcm : dc2 - dc1) - f.r * dden) / f.den;
            const T rp1 = T(1) + f.r;
            const T dphi = f.lim ? (T(2) * dr - f.phi * dr) / rp1 : T(0);
            const T dci = dclow - ((dclow - dchigh) * f.phi + f.cmh * dphi);
            return dci * f.w + f.ci * dw;
        }
    }
}

// The stencil of ONE momentum component around cell (i, j): the transported component C along both axes and the two cells
// behind each of its four face velocities.  COMP 0 is ux (its axis-0 faces move with ux itself, its axis-1 faces with uy), COMP 1
// is uy (the other way round): the faces and arguments of explicit_point / explicit_point_jvp.  The two-cell schemes never form
// the +-2 addresses.
template <typename T>
struct CompStencil {
    T c00, cm1, cp1, cm2, cp2, cjm1, cjp1, cjm2, cjp2;
    T fh_a, fh_b, fl_a, fl_b, gh_a, gh_b, gl_a, gl_b;
};

template <int COMP, int SCHEME, typename T>
__device__ __forceinline__ CompStencil<T> comp_stencil(const T* __restrict__ C, const T* __restrict__ O, int i, int j, int n) {
    auto at = [n](const T* p, int a, int b) { return p[(size_t)a * n + b]; };
    const int im1 = wrap(i - 1, n), ip1 = wrap(i + 1, n);
    const int jm1 = wrap(j - 1, n), jp1 = wrap(j + 1, n);
    CompStencil<T> v{};
    v.c00 = at(C, i, j);
    v.cm1 = at(C, im1, j);
    v.cp1 = at(C, ip1, j);
    v.cjm1 = at(C, i, jm1);
    v.cjp1 = at(C, i, jp1);
    if constexpr (SCHEME == VAN_LEER) {
        v.cm2 = at(C, wrap(i - 2, n), j);
        v.cp2 = at(C, wrap(i + 2, n), j);
        v.cjm2 = at(C, i, wrap(j - 2, n));
        v.cjp2 = at(C, i, wrap(j + 2, n));
    }
    if constexpr (COMP == 0) {
        v.fh_a = v.c00, v.fh_b = v.cp1;
        v.fl_a = v.cm1, v.fl_b = v.c00;
        v.gh_a = at(O, i, j), v.gh_b = at(O, ip1, j);
        v.gl_a = at(O, i, jm1), v.gl_b = at(O, ip1, jm1);
    } else {
        v.fh_a = at(O, i, j), v.fh_b = at(O, i, jp1);
        v.fl_a = at(O, im1, j), v.fl_b = at(O, im1, jp1);
        v.gh_a = v.c00, v.gh_b = v.cjp1;
        v.gl_a = v.cjm1, v.gl_b = v.c00;
    }
    return v;
}

// One momentum component of the K members of cell (i, j): the four faces' state shares once, then per member the tangent of
// explicit_point_jvp's component -- its fluxes, the order of its sums, finish_point's Laplacian and drag on the perturbation, no
// forcing -- and k_fvm_stage_jvp's target expressions.  U / U0 / K_OUT / tgp: this component's arrays; UO: the other component.
template <int COMP, int SCHEME, typename T, typename S>
__device__ __forceinline__ void bundle_component(const T* __restrict__ U, const T* __restrict__ UO, const T* __restrict__ U0,
                                                 T* __restrict__ K_OUT, T* const* tgp, const Targets<T>& tg, const S& s, int i,
                                                 int j, int n, size_t base, size_t tan_stride, int ntan) {
    FaceState<T> f_hi, f_lo, g_hi, g_lo;
    {
        const CompStencil<T> v = comp_stencil<COMP, SCHEME>(U + base, UO + base, i, j, n);
        f_hi = face_state<SCHEME>(v.cm1, v.c00, v.cp1, v.cp2, half(v.fh_a, v.fh_b), s.cfl);
        f_lo = face_state<SCHEME>(v.cm2, v.cm1, v.c00, v.cp1, half(v.fl_a, v.fl_b), s.cfl);
        g_hi = face_state<SCHEME>(v.cjm1, v.c00, v.cjp1, v.cjp2, half(v.gh_a, v.gh_b), s.cfl);
        g_lo = face_state<SCHEME>(v.cjm2, v.cjm1, v.c00, v.cjp1, half(v.gl_a, v.gl_b), s.cfl);
    }
    const size_t p = base + (size_t)i * n + j;
    for (int k = 0; k < ntan; ++k) {
        const size_t off = (size_t)(k + 1) * tan_stride;
        const CompStencil<T> d = comp_stencil<COMP, SCHEME>(U + off + base, UO + off + base, i, j, n);
        const T t_fhi = face_state_jvp<SCHEME>(f_hi, d.cm1, d.c00, d.cp1, d.cp2, half(d.fh_a, d.fh_b), s.cfl);
        const T t_flo = face_state_jvp<SCHEME>(f_lo, d.cm2, d.cm1, d.c00, d.cp1, half(d.fl_a, d.fl_b), s.cfl);
        const T t_ghi = face_state_jvp<SCHEME>(g_hi, d.cjm1, d.c00, d.cjp1, d.cjp2, half(d.gh_a, d.gh_b), s.cfl);
        const T t_glo = face_state_jvp<SCHEME>(g_lo, d.cjm2, d.cjm1, d.c00, d.cjp1, half(d.gl_a, d.gl_b), s.cfl);
        const T dadv = -((t_fhi - t_flo) / s.h + (t_ghi - t_glo) / s.h);
        // finish_point's component on the perturbation, without the forcing
        T lap = (T(-2) * d.c00) * s.sum_s;
        lap = lap + (d.cm1 + d.cp1) * s.inv_h2;
        lap = lap + (d.cjm1 + d.cjp1) * s.inv_h2;
        T dk = dadv + s.nu * lap;
        if (s.drag_on) dk = dk + d.c00 * s.neg_drag;
        const size_t dp = off + p;
        if (K_OUT) K_OUT[dp] = dk;
        for (int t = 0; t < tg.count; ++t) {
            const int mode = tg.mode[t];
            T v = mode == 2 ? tgp[t][dp] : U0[dp];
            if (mode != 3) v = v + dk * tg.c[t];
            tgp[t][dp] = v;
        }
    }
}

// k_fvm_stage_jvp for one state and its K = ntan perturbations: fields [0, B) of every array the state, fields
// [(1 + k) B, (2 + k) B) tangent k, `tan_stride` = B n^2 elements apart (K = 1: the pair layout).  One thread per cell of the B
// samples; blockIdx.z = sample; the thread walks the members, so nothing is summed across threads and two runs give the same
// bits.  The state half is explicit_point and k_fvm_stage's target expressions: the bits of the plain kernel.  The members go
// in two passes, the ux component of all K and then the uy component of all K, the two being independent down to their targets:
// a pass holds the state shares of four faces, not eight, across its member loop.
template <int SCHEME, typename T, typename S>
__global__ void __launch_bounds__(256) k_fvm_stage_jvp_bundle(const T* __restrict__ ux, const T* __restrict__ uy,
                                                              const T* __restrict__ u0x, const T* __restrict__ u0y,
                                                              const T* __restrict__ fx, const T* __restrict__ fy,
                                                              T* __restrict__ kx_out, T* __restrict__ ky_out, Targets<T> tg, S s,
                                                              int n, size_t tan_stride, int ntan) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t plane = (size_t)n * n;
    const size_t base = (size_t)blockIdx.z * plane;
    auto body = [&](const auto& c) {   // c: the constants of this sample (the plan's, or member blockIdx.z's for all 1 + K fields)
        T kx, ky;
        explicit_point<SCHEME>(ux + base, uy + base, fx, fy, i, j, n, c, kx, ky);
        const size_t p = base + (size_t)i * n + j;
        if (kx_out) {
            kx_out[p] = kx;
            ky_out[p] = ky;
        }
        for (int t = 0; t < tg.count; ++t) {
            const int mode = tg.mode[t];
            const T w = tg.c[t];
            T px, py;
            if (mode == 2) {
                px = tg.x[t][p];
                py = tg.y[t][p];
            } else {
                px = u0x[p];
                py = u0y[p];
            }
            if (mode != 3) {
                px = px + kx * w;
                py = py + ky * w;
            }
            tg.x[t][p] = px;
            tg.y[t][p] = py;
        }
        bundle_component<0, SCHEME>(ux, uy, u0x, kx_out, tg.x, tg, c, i, j, n, base, tan_stride, ntan);
        bundle_component<1, SCHEME>(uy, ux, u0y, ky_out, tg.y, tg, c, i, j, n, base, tan_stride, ntan);
    };
    if constexpr (kEnsemble<S>)
        body(member_const(s.plan, s.rows, blockIdx.z));
    else
        body(s);
}

// div = (ux - ux[i-1]) / h + (uy - uy[j-1]) / h  (finite_differences.py:116-135)
template <typename T>
__global__ void __launch_bounds__(256) k_fvm_div(const T* __restrict__ ux, const T* __restrict__ uy, T* __restrict__ div, T h, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t base = (size_t)blockIdx.z * n * n;
    const size_t p = base + (size_t)i * n + j;
    const T dx = (ux[p] - ux[base + (size_t)wrap(i - 1, n) * n + j]) / h;
    const T dy = (uy[p] - uy[base + (size_t)i * n + wrap(j - 1, n)]) / h;
    div[p] = dx + dy;
}

// spectrum *= inverse eigenvalues (pressure.py: multiplier * fft(value)), complex (re, im) pairs
template <typename T>
__global__ void __launch_bounds__(256) k_fvm_mul(T* __restrict__ spec, const T* __restrict__ inv, long plane, long total) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long t = e % plane;
    const T ar = inv[2 * t], ai = inv[2 * t + 1];
    const T br = spec[2 * e], bi = spec[2 * e + 1];
    spec[2 * e] = ar * br - ai * bi;
    spec[2 * e + 1] = ar * bi + ai * br;
}

// out = P - (q[+1] - q) / h per component (pressure.py:100-106 with forward_difference, finite_differences.py:69)
template <typename T>
__global__ void __launch_bounds__(256) k_fvm_apply(const T* __restrict__ px, const T* __restrict__ py, const T* __restrict__ q,
                                                   T* __restrict__ ox, T* __restrict__ oy, T h, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t base = (size_t)blockIdx.z * n * n;
    const size_t p = base + (size_t)i * n + j;
    const T q0 = q[p];
    const T gx = (q[base + (size_t)wrap(i + 1, n) * n + j] - q0) / h;
    const T gy = (q[base + (size_t)i * n + wrap(j + 1, n)] - q0) / h;
    ox[p] = px[p] - gx;
    oy[p] = py[p] - gy;
}

// ---------------------------------------------------------------- adjoint (vector-Jacobian products)
// The projection is symmetric (P = I - G pinv(L) D with D = -G^T, L = D G), so its VJP is the projection of the cotangent.
// The explicit terms' VJP is gathered: the thread of cell (i, j) recomputes the partial derivatives of every face flux whose
// stencil reads ux[i][j] or uy[i][j] and sums (cotangent of the flux) * (partial).  No atomics: the result is bitwise
// reproducible.

// cotangents of the inputs (cm, c0, c1, c2, w) of tvd_flux, given the cotangent lam of its result.  The derivative follows
// the branches torch autograd takes through the reference's ops: the selections w > 0 and r > 0 pass no gradient, w still
// enters through the Courant number and the final product; safe_div's constant denominator 1 (d == 0) takes none.
template <typename T>
struct FluxBar {
    T cm, c0, c1, c2, w;
};

template <typename T>
__device__ __forceinline__ FluxBar<T> tvd_flux_vjp(T cm, T c0, T c1, T c2, T w, T cfl, T lam) {
    const bool pos = w > T(0);
    const T clow = pos ? c0 : c1;
    const T cr = cfl * w;
    const T d = c1 - c0;
    const T alpha = T(0.5) * (T(1) - cr);   // hp = c0 + alpha d
    const T beta = T(0.5) * (T(1) + cr);    // hn = c1 - beta d
    const T chigh = pos ? c0 + alpha * d : c1 - beta * d;
    const bool dnz = d != T(0);
    const T dd = dnz ? d : T(1);
    const T r = (pos ? c0 - cm : c2 - c1) / dd;
    const bool lim = r > T(0);
    const T rp1 = T(1) + r;
    const T phi = lim ? (T(2) * r) / rp1 : T(0);
    const T dphi = lim ? T(2) / (rp1 * rp1) : T(0);
    const T ci = clow - (clow - chigh) * phi;
    // flux = ci w,  ci = clow (1 - phi) + chigh phi
    const T bci = lam * w;
    const T bclow = bci * (T(1) - phi);
    const T bchigh = bci * phi;
    const T br = -(bci * (clow - chigh)) * dphi;
    const T bnum = br / dd;
    T bd = dnz ? -(br * r) / dd : T(0);      // through the denominator of r
    FluxBar<T> g;
    g.w = lam * ci + bchigh * (T(-0.5) * cfl * d);   // d chigh / d w = -cfl d / 2 in both branches
    g.cm = T(0);
    g.c2 = T(0);
    if (pos) {
        g.c0 = bclow + bchigh + bnum;
        g.c1 = T(0);
        g.cm = -bnum;
        bd = bd + bchigh * alpha;
    } else {
        g.c0 = T(0);
        g.c1 = bclow + bchigh - bnum;
        g.c2 = bnum;
        bd = bd - bchigh * beta;
    }
    g.c1 = g.c1 + bd;
    g.c0 = g.c0 - bd;
    return g;
}

// cotangents of the inputs (c0, c1, w) of face_flux, given the cotangent lam of its result, by the same rules: the selection
// w > 0 passes no gradient (w == 0 takes the c1 branch, as the forward), w enters through the final product and, for
// LAX_WENDROFF, through the Courant number.
template <typename T>
struct FaceBar {
    T c0, c1, w;
};

template <int SCHEME, typename T>
__device__ __forceinline__ FaceBar<T> face_flux_vjp(T c0, T c1, T w, T cfl, T lam) {
    static_assert(SCHEME == UPWIND || SCHEME == LINEAR || SCHEME == LAX_WENDROFF, "two-cell schemes only");
    const T bci = lam * w;   // flux = ci w
    FaceBar<T> g;
    if constexpr (SCHEME == UPWIND) {
        const bool pos = w > T(0);
        g.w = lam * (pos ? c0 : c1);
        g.c0 = pos ? bci : T(0);
        g.c1 = pos ? T(0) : bci;
    } else if constexpr (SCHEME == LINEAR) {
        g.w = lam * half(c0, c1);
        g.c0 = bci * T(0.5);
        g.c1 = bci * T(0.5);
    } else {
        const bool pos = w > T(0);
        const T cr = cfl * w;
        const T d = c1 - c0;
        const T alpha = T(0.5) * (T(1) - cr);   // hp = c0 + alpha d
        const T beta = T(0.5) * (T(1) + cr);    // hn = c1 - beta d
        const T ci = pos ? c0 + alpha * d : c1 - beta * d;
        g.w = lam * ci + bci * (T(-0.5) * cfl * d);   // d ci / d w = -cfl d / 2 in both branches
        const T bd = pos ? bci * alpha : -(bci * beta);
        g.c0 = (pos ? bci : T(0)) - bd;
        g.c1 = (pos ? T(0) : bci) + bd;
    }
    return g;
}

// (lx, ly) = J^T (LX, LY) of explicit_point at cell (i, j): X / Y the state, LX / LY the cotangent of (kx, ky).
// Face fluxes (p, q any cell, all indices periodic):
//   FX[p][q] ux along axis 0: tvd_flux(X[p-1][q], X[p][q], X[p+1][q], X[p+2][q], half(X[p][q], X[p+1][q]))
//   GX[p][q] ux along axis 1: tvd_flux(X[p][q-1], X[p][q], X[p][q+1], X[p][q+2], half(Y[p][q], Y[p+1][q]))
//   FY[p][q] uy along axis 0: tvd_flux(Y[p-1][q], Y[p][q], Y[p+1][q], Y[p+2][q], half(X[p][q], X[p][q+1]))
//   GY[p][q] uy along axis 1: tvd_flux(Y[p][q-1], Y[p][q], Y[p][q+1], Y[p][q+2], half(Y[p][q], Y[p][q+1]))
// kx[p][q] = -((FX[p][q] - FX[p-1][q]) / h + (GX[p][q] - GX[p][q-1]) / h) + ..., so the cotangent of FX[p][q] is
// (LX[p+1][q] - LX[p][q]) / h, and likewise for the others.  X[i][j] is read by FX[i-2 .. i+1][j], GX[i][j-2 .. j+1] and
// the face velocities of FY[i][j-1 .. j]; Y[i][j] by FY[i-2 .. i+1][j], GY[i][j-2 .. j+1] and the face velocities of
// GX[i-1 .. i][j]: 18 flux evaluations per cell, against the forward's 8.
// The two-cell schemes' faces F(c0, c1, w) drop the cm and c2 arguments above: X[i][j] is the c1 of FX[i-1][j] and
// GX[i][j-1], the c0 of FX[i][j] and GX[i][j], and half of the face velocities of FX[i-1 .. i][j] and FY[i][j-1 .. j];
// Y[i][j] likewise.  The faces two cells away have identically zero partials and are not evaluated: 10 flux evaluations per
// cell (FY[i][j] and GX[i][j] serve both components), reading the 5-point stencils of X and Y, the corners (i-1, j+1) and
// (i+1, j-1) of both, the 5-point stencils of LX and LY, LX[i-1][j+1] and LY[i+1][j-1].
template <int SCHEME, typename T, typename S>
__device__ __forceinline__ void explicit_point_vjp(const T* __restrict__ X, const T* __restrict__ Y, const T* __restrict__ LX,
                                                   const T* __restrict__ LY, int i, int j, int n, const S& s, T& lx,
                                                   T& ly) {
    auto at = [n](const T* p, int a, int b) { return p[(size_t)wrap(a, n) * n + wrap(b, n)]; };
    auto cot = [&](const T* l, int a, int b, int a1, int b1) { return (at(l, a1, b1) - at(l, a, b)) / s.h; };
    T gx = T(0), gy = T(0);
    if constexpr (SCHEME == VAN_LEER) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // FX[p][j], p = i - 2 + k: X[i][j] is its c2, c1, c0, cm
            const int p = i - 2 + k;
            const T c0 = at(X, p, j), c1 = at(X, p + 1, j);
            const FluxBar<T> b = tvd_flux_vjp(at(X, p - 1, j), c0, c1, at(X, p + 2, j), half(c0, c1), s.cfl, cot(LX, p, j, p + 1, j));
            gx = gx + (k == 0 ? b.c2 : k == 1 ? b.c1 + T(0.5) * b.w : k == 2 ? b.c0 + T(0.5) * b.w : b.cm);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // GX[i][q], q = j - 2 + k; Y[i][j] is the first half of the face velocity of GX[i][j]
            const int q = j - 2 + k;
            const FluxBar<T> b = tvd_flux_vjp(at(X, i, q - 1), at(X, i, q), at(X, i, q + 1), at(X, i, q + 2),
                                              half(at(Y, i, q), at(Y, i + 1, q)), s.cfl, cot(LX, i, q, i, q + 1));
            gx = gx + (k == 0 ? b.c2 : k == 1 ? b.c1 : k == 2 ? b.c0 : b.cm);
            if (k == 2) gy = gy + T(0.5) * b.w;
        }
        {   // GX[i-1][j]: Y[i][j] is the second half of its face velocity
            const FluxBar<T> b = tvd_flux_vjp(at(X, i - 1, j - 1), at(X, i - 1, j), at(X, i - 1, j + 1), at(X, i - 1, j + 2),
                                              half(at(Y, i - 1, j), at(Y, i, j)), s.cfl, cot(LX, i - 1, j, i - 1, j + 1));
            gy = gy + T(0.5) * b.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // FY[p][j], p = i - 2 + k; X[i][j] is the first half of the face velocity of FY[i][j]
            const int p = i - 2 + k;
            const FluxBar<T> b = tvd_flux_vjp(at(Y, p - 1, j), at(Y, p, j), at(Y, p + 1, j), at(Y, p + 2, j),
                                              half(at(X, p, j), at(X, p, j + 1)), s.cfl, cot(LY, p, j, p + 1, j));
            gy = gy + (k == 0 ? b.c2 : k == 1 ? b.c1 : k == 2 ? b.c0 : b.cm);
            if (k == 2) gx = gx + T(0.5) * b.w;
        }
        {   // FY[i][j-1]: X[i][j] is the second half of its face velocity
            const FluxBar<T> b = tvd_flux_vjp(at(Y, i - 1, j - 1), at(Y, i, j - 1), at(Y, i + 1, j - 1), at(Y, i + 2, j - 1),
                                              half(at(X, i, j - 1), at(X, i, j)), s.cfl, cot(LY, i, j - 1, i + 1, j - 1));
            gx = gx + T(0.5) * b.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // GY[i][q], q = j - 2 + k
            const int q = j - 2 + k;
            const T c0 = at(Y, i, q), c1 = at(Y, i, q + 1);
            const FluxBar<T> b = tvd_flux_vjp(at(Y, i, q - 1), c0, c1, at(Y, i, q + 2), half(c0, c1), s.cfl, cot(LY, i, q, i, q + 1));
            gy = gy + (k == 0 ? b.c2 : k == 1 ? b.c1 + T(0.5) * b.w : k == 2 ? b.c0 + T(0.5) * b.w : b.cm);
        }
    } else {
        const T x00 = at(X, i, j), y00 = at(Y, i, j);
        const T xm1 = at(X, i - 1, j), xp1 = at(X, i + 1, j), xjm1 = at(X, i, j - 1), xjp1 = at(X, i, j + 1);
        const T ym1 = at(Y, i - 1, j), yp1 = at(Y, i + 1, j), yjm1 = at(Y, i, j - 1), yjp1 = at(Y, i, j + 1);
        {   // FX[i-1][j]: X[i][j] is its c1 and the second half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(xm1, x00, half(xm1, x00), s.cfl, cot(LX, i - 1, j, i, j));
            gx = gx + (b.c1 + T(0.5) * b.w);
        }
        {   // FX[i][j]: its c0 and the first half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(x00, xp1, half(x00, xp1), s.cfl, cot(LX, i, j, i + 1, j));
            gx = gx + (b.c0 + T(0.5) * b.w);
        }
        {   // GX[i][j-1]: X[i][j] is its c1
            const FaceBar<T> b = face_flux_vjp<SCHEME>(xjm1, x00, half(yjm1, at(Y, i + 1, j - 1)), s.cfl, cot(LX, i, j - 1, i, j));
            gx = gx + b.c1;
        }
        {   // GX[i][j]: X[i][j] is its c0, Y[i][j] the first half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(x00, xjp1, half(y00, yp1), s.cfl, cot(LX, i, j, i, j + 1));
            gx = gx + b.c0;
            gy = gy + T(0.5) * b.w;
        }
        {   // GX[i-1][j]: Y[i][j] is the second half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(xm1, at(X, i - 1, j + 1), half(ym1, y00), s.cfl, cot(LX, i - 1, j, i - 1, j + 1));
            gy = gy + T(0.5) * b.w;
        }
        {   // FY[i-1][j]: Y[i][j] is its c1
            const FaceBar<T> b = face_flux_vjp<SCHEME>(ym1, y00, half(xm1, at(X, i - 1, j + 1)), s.cfl, cot(LY, i - 1, j, i, j));
            gy = gy + b.c1;
        }
        {   // FY[i][j]: Y[i][j] is its c0, X[i][j] the first half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(y00, yp1, half(x00, xjp1), s.cfl, cot(LY, i, j, i + 1, j));
            gy = gy + b.c0;
            gx = gx + T(0.5) * b.w;
        }
        {   // FY[i][j-1]: X[i][j] is the second half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(yjm1, at(Y, i + 1, j - 1), half(xjm1, x00), s.cfl, cot(LY, i, j - 1, i + 1, j - 1));
            gx = gx + T(0.5) * b.w;
        }
        {   // GY[i][j-1]: Y[i][j] is its c1 and the second half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(yjm1, y00, half(yjm1, y00), s.cfl, cot(LY, i, j - 1, i, j));
            gy = gy + (b.c1 + T(0.5) * b.w);
        }
        {   // GY[i][j]: its c0 and the first half of its face velocity
            const FaceBar<T> b = face_flux_vjp<SCHEME>(y00, yjp1, half(y00, yjp1), s.cfl, cot(LY, i, j, i, j + 1));
            gy = gy + (b.c0 + T(0.5) * b.w);
        }
    }
    // the 5-point Laplacian is symmetric: nu lap(L); drag: -drag L; the forcing does not depend on the state
    const T l00x = at(LX, i, j), l00y = at(LY, i, j);
    T lap_x = (T(-2) * l00x) * s.sum_s;
    lap_x = lap_x + (at(LX, i - 1, j) + at(LX, i + 1, j)) * s.inv_h2;
    lap_x = lap_x + (at(LX, i, j - 1) + at(LX, i, j + 1)) * s.inv_h2;
    T lap_y = (T(-2) * l00y) * s.sum_s;
    lap_y = lap_y + (at(LY, i - 1, j) + at(LY, i + 1, j)) * s.inv_h2;
    lap_y = lap_y + (at(LY, i, j - 1) + at(LY, i, j + 1)) * s.inv_h2;
    lx = gx + s.nu * lap_x;
    ly = gy + s.nu * lap_y;
    if (s.drag_on) {
        lx = lx + l00x * s.neg_drag;
        ly = ly + l00y * s.neg_drag;
    }
}

// (ox, oy) = J_F(u)^T (lx, ly), or += with accumulate (stage 0 of the reverse step adds straight into the cotangent of u0)
template <int SCHEME, typename T, typename S>
__global__ void __launch_bounds__(256) k_fvm_stage_vjp(const T* __restrict__ ux, const T* __restrict__ uy, const T* __restrict__ lx,
                                                       const T* __restrict__ ly, T* __restrict__ ox, T* __restrict__ oy,
                                                       int accumulate, S s, int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t base = (size_t)blockIdx.z * n * n;
    T gx, gy;
    if constexpr (kEnsemble<S>)   // the cotangent of sample blockIdx.z is pulled back through member blockIdx.z's Jacobian
        explicit_point_vjp<SCHEME>(ux + base, uy + base, lx + base, ly + base, i, j, n, member_const(s.plan, s.rows, blockIdx.z), gx, gy);
    else
        explicit_point_vjp<SCHEME>(ux + base, uy + base, lx + base, ly + base, i, j, n, s, gx, gy);
    const size_t p = base + (size_t)i * n + j;
    if (accumulate) {
        gx = ox[p] + gx;
        gy = oy[p] + gy;
    }
    ox[p] = gx;
    oy[p] = gy;
}

constexpr int MAXA = MAXT + 1;   // targets of an adjoint apply: the cotangent of u0 + one per stage

template <typename T>
struct AdjTargets {
    T* x[MAXA];
    T* y[MAXA];
    T c[MAXA];
    int mode[MAXA];   // 0: t = mu,  1: t = t + mu,  2: t = mu * c,  3: t = t + mu * c
    int count;
};

// mu = g - grad q (the projection's apply pass on a cotangent), then every target (+)= (c) mu.  A target may alias g.
template <typename T>
__global__ void __launch_bounds__(256) k_fvm_apply_adj(const T* gx, const T* gy, const T* __restrict__ q, AdjTargets<T> tg, T h,
                                                       int n) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t base = (size_t)blockIdx.z * n * n;
    const size_t p = base + (size_t)i * n + j;
    const T q0 = q[p];
    const T mx = gx[p] - (q[base + (size_t)wrap(i + 1, n) * n + j] - q0) / h;
    const T my = gy[p] - (q[base + (size_t)i * n + wrap(j + 1, n)] - q0) / h;
    for (int t = 0; t < tg.count; ++t) {
        const int mode = tg.mode[t];
        T vx = mode >= 2 ? mx * tg.c[t] : mx;
        T vy = mode >= 2 ? my * tg.c[t] : my;
        if (mode & 1) {
            vx = tg.x[t][p] + vx;
            vy = tg.y[t][p] + vy;
        }
        tg.x[t][p] = vx;
        tg.y[t][p] = vy;
    }
}

}  // namespace

struct tcfd_fvm_plan {
    int n;
    int dtype;                 // TCFD_C128: fp64 fields, TCFD_C64: fp32
    double h, nu, drag;
    tcfd_ns2d_plan* fft;       // table-free spectral plan: the rfft2 / irfft2 kernels
    void* inv;                 // (n, n/2 + 1) complex inverse eigenvalues, field precision
    void* fx;                  // (n, n) forcing / density per component, field precision (NULL: no forcing)
    void* fy;
    size_t fft_ws;             // tcfd_ns2d_workspace_bytes of the transform plan, per batch, computed at call time
    int scheme;                // TCFD_FVM_*: the instantiation of k_fvm_stage / k_fvm_stage_vjp, read at every launch
    int tangent;               // 1: every call carries pairs, fields [0, B) the state and [B, 2 B) its perturbation
    void* ens;                 // per-sample physics (tcfd_fvm_plan_set_ensemble): ens_count x {nu / density, -drag, forcing scale}
    long ens_count;            //   in the field precision, or NULL / 0: a scalar plan, whose launches are what they always were
    int bundle;                // K > 0: every call carries 1 + K fields per sample, the state and K perturbations of it (excludes tangent)
};

namespace {

// ---- launchers, templates on the field type T; the C ABI dispatches on the plan's dtype
dim3 cell_grid(int n, long batch) { return dim3((unsigned)((n + 63) / 64), (unsigned)((n + 3) / 4), (unsigned)batch); }
const dim3 kCellBlock(64, 4, 1);

template <typename T>
StageConst<T> stage_const(const tcfd_fvm_plan* p, double dt) {
    StageConst<T> s;
    const double inv_h2 = 1.0 / (p->h * p->h);
    s.cfl = (T)(dt / p->h);
    s.inv_h2 = (T)inv_h2;
    s.sum_s = (T)(inv_h2 + inv_h2);
    s.nu = (T)p->nu;
    s.neg_drag = (T)(-p->drag);
    s.h = (T)p->h;
    s.drag_on = p->drag > 0.0;
    return s;
}

// an ensemble plan steps exactly its own members, one field each (a tangent plan: the state and the perturbation of each).  Every
// entry point that evaluates the explicit terms checks it before it touches the device, and the two stage launchers check it
// again: row blockIdx.z of the table exists for every block they launch.
int check_ensemble_batch(const tcfd_fvm_plan* p, long batch, const char* what) {
    if (p->ens_count <= 0) return 0;
    if (p->bundle) {
        if (batch != (1 + (long)p->bundle) * p->ens_count)
            return FAIL(TCFD_EINVAL, "%s: batch %ld on a bundle plan of %d tangents with per-sample parameters for %ld members, which "
                                     "takes (1 + %d) x %ld fields (tcfd_fvm_plan_set_ensemble)", what, batch, p->bundle, p->ens_count,
                        p->bundle, p->ens_count);
        return 0;
    }
    if (p->tangent && batch != 2 * p->ens_count)
        return FAIL(TCFD_EINVAL, "%s: batch %ld on a tangent plan with per-sample parameters for %ld members, which takes 2 x %ld "
                                 "fields (tcfd_fvm_plan_set_ensemble)", what, batch, p->ens_count, p->ens_count);
    if (!p->tangent && batch != p->ens_count)
        return FAIL(TCFD_EINVAL, "%s: batch %ld on a plan with per-sample parameters for %ld fields (tcfd_fvm_plan_set_ensemble)",
                    what, batch, p->ens_count);
    return 0;
}

// a bundle plan steps whole bundles, 1 + K fields per sample, and every pass but the stage kernel puts the field index in
// gridDim.z (cell_grid): checked by every entry point that takes a bundle before it touches the device, and by the stage launcher
constexpr long kMaxGridZ = 65535;

int check_bundle_batch(const tcfd_fvm_plan* p, long batch, const char* what) {
    if (!p->bundle) return 0;
    if (batch % (1 + (long)p->bundle))
        return FAIL(TCFD_EINVAL, "%s: batch %ld on a bundle plan of %d tangents, which takes whole bundles (batch = (1 + %d) B)", what,
                    batch, p->bundle, p->bundle);
    if (batch > kMaxGridZ)
        return FAIL(TCFD_EINVAL, "%s: %ld fields on a bundle plan of %d tangents: the launch grids take at most %ld fields (state and "
                                 "tangents together) in one call", what, batch, p->bundle, kMaxGridZ);
    return 0;
}

template <typename T>
int stage_launch(const tcfd_fvm_plan* p, const void* ux, const void* uy, const void* u0x, const void* u0y, void* kx, void* ky,
                 void* const* tx, void* const* ty, const double* c, const int* mode, int count, long batch, double dt,
                 hipStream_t st) {
    if (int rc = check_bundle_batch(p, batch, "fvm stage")) return rc;
    if (int rc = check_ensemble_batch(p, batch, "fvm stage")) return rc;
    Targets<T> tg;
    tg.count = count;
    for (int t = 0; t < MAXT; ++t) {
        tg.x[t] = t < count ? (T*)tx[t] : nullptr;
        tg.y[t] = t < count ? (T*)ty[t] : nullptr;
        tg.c[t] = t < count ? (T)c[t] : T(0);
        tg.mode[t] = t < count ? mode[t] : 0;
    }
    // a tangent plan: the pair kernel over the B = batch / 2 samples, the perturbation B planes after the state
    const long half_batch = batch / 2;
    const size_t pair = (size_t)half_batch * p->n * p->n;
    // an ensemble plan: the EnsConst instantiations on the member table.  No call splits its batch, so sample 0 of a launch is member 0.
    const T* ens = (const T*)p->ens;
    // a bundle plan: the bundle kernel over the B = batch / (1 + K) samples, tangent k (1 + k) B planes after the state
    const long samples = batch / (1 + (long)p->bundle);
    const size_t tan_stride = (size_t)samples * p->n * p->n;
#define STAGE(SCHEME)                                                                                                      \
    if (ens && p->bundle)                                                                                                  \
        hipLaunchKernelGGL((k_fvm_stage_jvp_bundle<SCHEME, T, EnsConst<T>>), cell_grid(p->n, samples), kCellBlock, 0, st,  \
                           (const T*)ux, (const T*)uy, (const T*)u0x, (const T*)u0y, (const T*)p->fx, (const T*)p->fy,     \
                           (T*)kx, (T*)ky, tg, EnsConst<T>{stage_const<T>(p, dt), ens}, p->n, tan_stride, p->bundle);      \
    else if (p->bundle)                                                                                                    \
        hipLaunchKernelGGL((k_fvm_stage_jvp_bundle<SCHEME, T, StageConst<T>>), cell_grid(p->n, samples), kCellBlock, 0, st, \
                           (const T*)ux, (const T*)uy, (const T*)u0x, (const T*)u0y, (const T*)p->fx, (const T*)p->fy,     \
                           (T*)kx, (T*)ky, tg, stage_const<T>(p, dt), p->n, tan_stride, p->bundle);                        \
    else if (ens && p->tangent)                                                                                                 \
        hipLaunchKernelGGL((k_fvm_stage_jvp<SCHEME, T, EnsConst<T>>), cell_grid(p->n, half_batch), kCellBlock, 0, st,      \
                           (const T*)ux, (const T*)uy, (const T*)u0x, (const T*)u0y, (const T*)p->fx, (const T*)p->fy,     \
                           (T*)kx, (T*)ky, tg, EnsConst<T>{stage_const<T>(p, dt), ens}, p->n, pair);                       \
    else if (ens)                                                                                                          \
        hipLaunchKernelGGL((k_fvm_stage<SCHEME, T, EnsConst<T>>), cell_grid(p->n, batch), kCellBlock, 0, st, (const T*)ux, \
                           (const T*)uy, (const T*)u0x, (const T*)u0y, (const T*)p->fx, (const T*)p->fy, (T*)kx, (T*)ky,   \
                           tg, EnsConst<T>{stage_const<T>(p, dt), ens}, p->n);                                             \
    else if (p->tangent)                                                                                                   \
        hipLaunchKernelGGL((k_fvm_stage_jvp<SCHEME, T, StageConst<T>>), cell_grid(p->n, half_batch), kCellBlock, 0, st, (const T*)ux, \
                           (const T*)uy, (const T*)u0x, (const T*)u0y, (const T*)p->fx, (const T*)p->fy, (T*)kx, (T*)ky,   \
                           tg, stage_const<T>(p, dt), p->n, pair);                                                         \
    else                                                                                                                   \
        hipLaunchKernelGGL((k_fvm_stage<SCHEME, T, StageConst<T>>), cell_grid(p->n, batch), kCellBlock, 0, st, (const T*)ux, \
                           (const T*)uy, (const T*)u0x, (const T*)u0y, (const T*)p->fx, (const T*)p->fy, (T*)kx, (T*)ky,   \
                           tg, stage_const<T>(p, dt), p->n)
    switch (p->scheme) {
        case VAN_LEER: STAGE(VAN_LEER); break;
        case UPWIND: STAGE(UPWIND); break;
        case LINEAR: STAGE(LINEAR); break;
        case LAX_WENDROFF: STAGE(LAX_WENDROFF); break;
        default: return FAIL(TCFD_EINVAL, "fvm: advection scheme %d", p->scheme);
    }
#undef STAGE
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int div_launch(const tcfd_fvm_plan* p, const void* ux, const void* uy, void* div, long batch, hipStream_t st) {
    hipLaunchKernelGGL(k_fvm_div<T>, cell_grid(p->n, batch), kCellBlock, 0, st, (const T*)ux, (const T*)uy, (T*)div, (T)p->h,
                       p->n);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int mul_launch(const tcfd_fvm_plan* p, void* spec, long batch, hipStream_t st) {
    const long plane = (long)p->n * (p->n / 2 + 1);
    const long total = plane * batch;
    hipLaunchKernelGGL(k_fvm_mul<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (T*)spec, (const T*)p->inv, plane,
                       total);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int apply_launch(const tcfd_fvm_plan* p, const void* px, const void* py, const void* q, void* ox, void* oy, long batch,
                 hipStream_t st) {
    hipLaunchKernelGGL(k_fvm_apply<T>, cell_grid(p->n, batch), kCellBlock, 0, st, (const T*)px, (const T*)py, (const T*)q,
                       (T*)ox, (T*)oy, (T)p->h, p->n);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int stage_vjp_launch(const tcfd_fvm_plan* p, const void* ux, const void* uy, const void* lx, const void* ly, void* ox, void* oy,
                     int accumulate, long batch, double dt, hipStream_t st) {
    if (int rc = check_ensemble_batch(p, batch, "fvm stage vjp")) return rc;
    const T* ens = (const T*)p->ens;
#define STAGE_VJP(SCHEME)                                                                                                  \
    if (ens)                                                                                                               \
        hipLaunchKernelGGL((k_fvm_stage_vjp<SCHEME, T, EnsConst<T>>), cell_grid(p->n, batch), kCellBlock, 0, st,           \
                           (const T*)ux, (const T*)uy, (const T*)lx, (const T*)ly, (T*)ox, (T*)oy, accumulate,             \
                           EnsConst<T>{stage_const<T>(p, dt), ens}, p->n);                                                 \
    else                                                                                                                   \
        hipLaunchKernelGGL((k_fvm_stage_vjp<SCHEME, T, StageConst<T>>), cell_grid(p->n, batch), kCellBlock, 0, st, (const T*)ux, \
                           (const T*)uy, (const T*)lx, (const T*)ly, (T*)ox, (T*)oy, accumulate, stage_const<T>(p, dt), p->n)
    switch (p->scheme) {
        case VAN_LEER: STAGE_VJP(VAN_LEER); break;
        case UPWIND: STAGE_VJP(UPWIND); break;
        case LINEAR: STAGE_VJP(LINEAR); break;
        case LAX_WENDROFF: STAGE_VJP(LAX_WENDROFF); break;
        default: return FAIL(TCFD_EINVAL, "fvm: advection scheme %d", p->scheme);
    }
#undef STAGE_VJP
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int apply_adj_launch(const tcfd_fvm_plan* p, const void* gx, const void* gy, const void* q, void* const* tx, void* const* ty,
                     const double* c, const int* mode, int count, long batch, hipStream_t st) {
    AdjTargets<T> tg;
    tg.count = count;
    for (int t = 0; t < MAXA; ++t) {
        tg.x[t] = t < count ? (T*)tx[t] : nullptr;
        tg.y[t] = t < count ? (T*)ty[t] : nullptr;
        tg.c[t] = t < count ? (T)c[t] : T(0);
        tg.mode[t] = t < count ? mode[t] : 0;
    }
    hipLaunchKernelGGL(k_fvm_apply_adj<T>, cell_grid(p->n, batch), kCellBlock, 0, st, (const T*)gx, (const T*)gy, (const T*)q,
                       tg, (T)p->h, p->n);
    HIP_TRY(hipGetLastError());
    return 0;
}

bool is_f64(const tcfd_fvm_plan* p) { return p->dtype == TCFD_C128; }
size_t real_bytes(const tcfd_fvm_plan* p) { return is_f64(p) ? 8 : 4; }
size_t field_bytes(const tcfd_fvm_plan* p, long batch) { return (size_t)batch * p->n * p->n * real_bytes(p); }
size_t spec_bytes(const tcfd_fvm_plan* p, long batch) { return (size_t)batch * p->n * (p->n / 2 + 1) * 2 * real_bytes(p); }

// ================================================================ C ABI
// the launchers above, instantiated by the plan's dtype
int stage_launch(const tcfd_fvm_plan* p, const void* ux, const void* uy, const void* u0x, const void* u0y, void* kx, void* ky,
                 void* const* tx, void* const* ty, const double* c, const int* mode, int count, long batch, double dt,
                 hipStream_t st) {
    return is_f64(p) ? stage_launch<double>(p, ux, uy, u0x, u0y, kx, ky, tx, ty, c, mode, count, batch, dt, st)
                     : stage_launch<float>(p, ux, uy, u0x, u0y, kx, ky, tx, ty, c, mode, count, batch, dt, st);
}
int apply_launch(const tcfd_fvm_plan* p, const void* px, const void* py, const void* q, void* ox, void* oy, long batch,
                 hipStream_t st) {
    return is_f64(p) ? apply_launch<double>(p, px, py, q, ox, oy, batch, st) : apply_launch<float>(p, px, py, q, ox, oy, batch, st);
}
int stage_vjp_launch(const tcfd_fvm_plan* p, const void* ux, const void* uy, const void* lx, const void* ly, void* ox, void* oy,
                     int accumulate, long batch, double dt, hipStream_t st) {
    return is_f64(p) ? stage_vjp_launch<double>(p, ux, uy, lx, ly, ox, oy, accumulate, batch, dt, st)
                     : stage_vjp_launch<float>(p, ux, uy, lx, ly, ox, oy, accumulate, batch, dt, st);
}
int apply_adj_launch(const tcfd_fvm_plan* p, const void* gx, const void* gy, const void* q, void* const* tx, void* const* ty,
                     const double* c, const int* mode, int count, long batch, hipStream_t st) {
    return is_f64(p) ? apply_adj_launch<double>(p, gx, gy, q, tx, ty, c, mode, count, batch, st)
                     : apply_adj_launch<float>(p, gx, gy, q, tx, ty, c, mode, count, batch, st);
}

// workspace carve: [div | spectrum | q | transform scratch] for the projection, then the RK buffers of tcfd_fvm_step, or
// those of tcfd_fvm_step_vjp: the stage states u_1 .. u_3, the stage cotangents kbar_0 .. kbar_3 and one g_i
struct Carve {
    void *div, *spec, *q, *fftws;
    size_t fftws_bytes;
    void *u0x, *u0y, *ucx, *ucy;
    void *px[MAXT], *py[MAXT];
    void *usx[MAXT - 1], *usy[MAXT - 1], *kbx[MAXT], *kby[MAXT], *gbx, *gby;
    size_t total;
};

constexpr int kProject = 0, kStep = 1, kStepVjp = 2;

Carve carve(const tcfd_fvm_plan* p, long batch, void* ws, int kind) {
    Carve c{};
    char* b = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* r = b ? b + off : nullptr;
        off += align256(bytes);
        return r;
    };
    const size_t F = field_bytes(p, batch);
    c.div = take(F);
    c.spec = take(spec_bytes(p, batch));
    c.q = take(F);
    c.fftws_bytes = tcfd_ns2d_workspace_bytes(p->fft, batch);
    c.fftws = take(c.fftws_bytes);
    if (kind == kStep) {
        c.u0x = take(F);
        c.u0y = take(F);
        c.ucx = take(F);
        c.ucy = take(F);
        for (int t = 0; t < MAXT; ++t) {
            c.px[t] = take(F);
            c.py[t] = take(F);
        }
    } else if (kind == kStepVjp) {
        for (int t = 0; t < MAXT - 1; ++t) {
            c.usx[t] = take(F);
            c.usy[t] = take(F);
        }
        for (int t = 0; t < MAXT; ++t) {
            c.kbx[t] = take(F);
            c.kby[t] = take(F);
        }
        c.gbx = take(F);
        c.gby = take(F);
    }
    c.total = off;
    return c;
}

// q of the field (px, py) into c.q
int solve_q(const tcfd_fvm_plan* p, const void* px, const void* py, long batch, const Carve& c, hipStream_t st) {
    int rc = is_f64(p) ? div_launch<double>(p, px, py, c.div, batch, st) : div_launch<float>(p, px, py, c.div, batch, st);
    if (rc) return rc;
    if ((rc = tcfd_rfft2(p->fft, c.div, c.spec, batch, st))) return rc;
    rc = is_f64(p) ? mul_launch<double>(p, c.spec, batch, st) : mul_launch<float>(p, c.spec, batch, st);
    if (rc) return rc;
    return tcfd_irfft2(p->fft, c.spec, c.q, batch, c.fftws, c.fftws_bytes, st);
}

int check_ws(const tcfd_fvm_plan* p, long batch, void* ws, size_t ws_bytes, int kind) {
    const size_t need = carve(p, batch, nullptr, kind).total;
    if (!ws || ws_bytes < need) return FAIL(TCFD_EWORKSPACE, "fvm: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 0;
}

}  // namespace

extern "C" {

int tcfd_fvm_plan_create(tcfd_fvm_plan** out, int n, int dtype, double h, double nu_over_density, double drag,
                                      const double* inverse_eig, const double* force_x, const double* force_y) {
    if (!out || !inverse_eig) return FAIL(TCFD_EINVAL, "fvm_plan_create: null argument");
    *out = nullptr;
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return FAIL(TCFD_EINVAL, "fvm_plan_create: dtype %d", dtype);
    if (!(h > 0.0)) return FAIL(TCFD_EINVAL, "fvm_plan_create: cell size %g", h);
    if ((force_x == nullptr) != (force_y == nullptr)) return FAIL(TCFD_EINVAL, "fvm_plan_create: give both forcing components or none");
    const int m = n / 2 + 1;
    std::vector<double> zx(n, 0.0), zy(m, 0.0), lin((size_t)n * m, 0.0), mask((size_t)n * m, 1.0);
    tcfd_ns2d_plan* fft = nullptr;
    int rc = tcfd_ns2d_plan_create(&fft, n, dtype, zx.data(), zy.data(), lin.data(), mask.data(), nullptr);
    if (rc) return rc;   // (the transform plan's message names the unsupported size)
    tcfd_fvm_plan* p = new tcfd_fvm_plan{};
    p->n = n;
    p->dtype = dtype;
    p->h = h;
    p->nu = nu_over_density;
    p->drag = drag;
    p->fft = fft;
    p->scheme = TCFD_FVM_VAN_LEER;
    const bool f64 = dtype == TCFD_C128;
    auto upload = [&](const double* src, size_t count, void** dst) -> int {
        const size_t bytes = count * (f64 ? 8 : 4);
        if (hipMalloc(dst, bytes) != hipSuccess) return FAIL(TCFD_ENOMEM, "fvm_plan_create: hipMalloc(%zu)", bytes);
        hipError_t e;
        if (f64) {
            e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        } else {
            std::vector<float> tmp(count);
            for (size_t k = 0; k < count; ++k) tmp[k] = (float)src[k];
            e = hipMemcpy(*dst, tmp.data(), bytes, hipMemcpyHostToDevice);
        }
        return e == hipSuccess ? 0 : FAIL(TCFD_EHIP, "fvm_plan_create: upload: %s", hipGetErrorString(e));
    };
    rc = upload(inverse_eig, (size_t)2 * n * m, &p->inv);
    if (!rc && force_x) rc = upload(force_x, (size_t)n * n, &p->fx);
    if (!rc && force_y) rc = upload(force_y, (size_t)n * n, &p->fy);
    if (rc) {
        tcfd_fvm_plan_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

void tcfd_fvm_plan_destroy(tcfd_fvm_plan* p) {
    if (!p) return;
    if (p->inv) (void)hipFree(p->inv);
    if (p->fx) (void)hipFree(p->fx);
    if (p->fy) (void)hipFree(p->fy);
    if (p->ens) (void)hipFree(p->ens);
    if (p->fft) tcfd_ns2d_plan_destroy(p->fft);
    delete p;
}

int tcfd_fvm_plan_set_advection(tcfd_fvm_plan* p, int scheme) {
    if (scheme != TCFD_FVM_VAN_LEER && scheme != TCFD_FVM_UPWIND && scheme != TCFD_FVM_LINEAR && scheme != TCFD_FVM_LAX_WENDROFF)
        return FAIL(TCFD_EINVAL, "fvm_plan_set_advection: unknown advection scheme %d (TCFD_FVM_VAN_LEER = 0, TCFD_FVM_UPWIND = 1, "
                                 "TCFD_FVM_LINEAR = 2, TCFD_FVM_LAX_WENDROFF = 3)", scheme);
    if (!p) return FAIL(TCFD_EINVAL, "fvm_plan_set_advection: null plan");
    p->scheme = scheme;
    return 0;
}

int tcfd_fvm_plan_set_tangent(tcfd_fvm_plan* p, int on) {
    if (on != 0 && on != 1) return FAIL(TCFD_EINVAL, "fvm_plan_set_tangent: on = %d (0: plain plan, 1: tangent plan)", on);
    if (!p) return FAIL(TCFD_EINVAL, "fvm_plan_set_tangent: null plan");
    if (on && p->bundle)
        return FAIL(TCFD_EINVAL, "fvm_plan_set_tangent: the plan is a bundle plan of %d tangents (tcfd_fvm_plan_set_tangent_bundle); "
                                 "clear the bundle first", p->bundle);
    p->tangent = on;
    return 0;
}

int tcfd_fvm_plan_set_tangent_bundle(tcfd_fvm_plan* p, int ntangents) {
    if (!p) return FAIL(TCFD_EINVAL, "fvm_plan_set_tangent_bundle: null plan");
    if (ntangents < 0 || ntangents > TCFD_FVM_MAX_TANGENTS)
        return FAIL(TCFD_EINVAL, "fvm_plan_set_tangent_bundle: ntangents = %d outside 0 .. %d (0: no bundle)", ntangents,
                    TCFD_FVM_MAX_TANGENTS);
    if (ntangents && p->tangent)
        return FAIL(TCFD_EINVAL, "fvm_plan_set_tangent_bundle: the plan is a tangent plan (tcfd_fvm_plan_set_tangent); clear it first");
    p->bundle = ntangents;
    return 0;
}

int tcfd_fvm_plan_set_ensemble(tcfd_fvm_plan* p, long count, const double* nu_over_density, const double* drag,
                               const double* forcing_scale) {
    if (!p) return FAIL(TCFD_EINVAL, "fvm_plan_set_ensemble: null plan");
    if (count < 0) return FAIL(TCFD_EINVAL, "fvm_plan_set_ensemble: count %ld < 0", count);
    if (count > 0 && !nu_over_density) return FAIL(TCFD_EINVAL, "fvm_plan_set_ensemble: nu_over_density is required when count > 0");
    if (count > 0 && forcing_scale && !p->fx)
        return FAIL(TCFD_EINVAL, "fvm_plan_set_ensemble: forcing scales on a plan without forcing tables (nothing to scale)");
    void* table = nullptr;
    if (count > 0) {
        // the rows in the field precision, each value converted as stage_const converts the plan's scalars
        const bool f64 = is_f64(p);
        const size_t values = (size_t)count * ENS_ROW, bytes = values * real_bytes(p);
        std::vector<double> rows(values);
        for (long b = 0; b < count; ++b) {
            rows[ENS_ROW * b + 0] = nu_over_density[b];
            rows[ENS_ROW * b + 1] = -(drag ? drag[b] : p->drag);
            rows[ENS_ROW * b + 2] = forcing_scale ? forcing_scale[b] : 1.0;
        }
        std::vector<float> rows32;
        if (!f64) rows32.assign(rows.begin(), rows.end());
        if (hipMalloc(&table, bytes) != hipSuccess) return FAIL(TCFD_ENOMEM, "fvm_plan_set_ensemble: hipMalloc(%zu)", bytes);
        const hipError_t e = hipMemcpy(table, f64 ? (const void*)rows.data() : (const void*)rows32.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {   // set whole or not at all: the plan keeps the table it had
            (void)hipFree(table);
            return FAIL(TCFD_EHIP, "fvm_plan_set_ensemble: upload: %s", hipGetErrorString(e));
        }
    }
    // (hipFree waits for the device: no launch of an earlier call still reads the old table)
    if (p->ens) (void)hipFree(p->ens);
    p->ens = table;
    p->ens_count = count;
    return 0;
}

size_t tcfd_fvm_workspace_bytes(const tcfd_fvm_plan* p, long batch) {
    if (!p || batch <= 0) return 0;
    return carve(p, batch, nullptr, kStep).total;
}

int tcfd_fvm_explicit_terms(const tcfd_fvm_plan* p, const void* ux, const void* uy, void* kx, void* ky, long batch,
                                         double dt, void* stream) {
    if (!p || !ux || !uy || !kx || !ky || batch <= 0) return FAIL(TCFD_EINVAL, "fvm_explicit_terms: bad argument");
    if (p->tangent && batch % 2)
        return FAIL(TCFD_EINVAL, "fvm_explicit_terms: batch %ld on a tangent plan, which takes pairs (batch = 2 B)", batch);
    if (int rcb = check_bundle_batch(p, batch, "fvm_explicit_terms")) return rcb;
    if (int rce = check_ensemble_batch(p, batch, "fvm_explicit_terms")) return rce;
    return stage_launch(p, ux, uy, ux, uy, kx, ky, nullptr, nullptr, nullptr, nullptr, 0, batch, dt, (hipStream_t)stream);
}

int tcfd_fvm_project(const tcfd_fvm_plan* p, const void* ux, const void* uy, void* ux_out, void* uy_out, long batch,
                                  void* ws, size_t ws_bytes, void* stream) {
    if (!p || !ux || !uy || !ux_out || !uy_out || batch <= 0) return FAIL(TCFD_EINVAL, "fvm_project: bad argument");
    int rc = check_ws(p, batch, ws, ws_bytes, kProject);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Carve c = carve(p, batch, ws, kProject);
    if ((rc = solve_q(p, ux, uy, batch, c, st))) return rc;
    return apply_launch(p, ux, uy, c.q, ux_out, uy_out, batch, st);
}

int tcfd_fvm_step(const tcfd_fvm_plan* p, const void* ux_in, const void* uy_in, void* ux_out, void* uy_out,
                               long batch, int steps, int nstages, const double* a, const double* b, double dt, void* ws,
                               size_t ws_bytes, void* stream) {
    if (!p || !ux_in || !uy_in || !ux_out || !uy_out || batch <= 0 || steps < 0 || !b || (nstages > 1 && !a))
        return FAIL(TCFD_EINVAL, "fvm_step: bad argument");
    if (p->tangent && batch % 2)
        return FAIL(TCFD_EINVAL, "fvm_step: batch %ld on a tangent plan, which takes pairs (batch = 2 B)", batch);
    if (int rcb = check_bundle_batch(p, batch, "fvm_step")) return rcb;
    if (int rce = check_ensemble_batch(p, batch, "fvm_step")) return rce;
    if (nstages < 1 || nstages > MAXT) return FAIL(TCFD_EINVAL, "fvm_step: %d stages (1 .. %d supported)", nstages, MAXT);
    for (int i = 0; i < nstages; ++i)
        for (int j = i; j < nstages; ++j)
            if (nstages > 1 && a[i * nstages + j] != 0.0)
                return FAIL(TCFD_EINVAL, "fvm_step: a[%d][%d] != 0: only explicit (strictly lower) tableaux", i, j);
    int rc = check_ws(p, batch, ws, ws_bytes, kStep);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Carve c = carve(p, batch, ws, kStep);
    const size_t F = field_bytes(p, batch);
    if (steps == 0) {
        if (ux_out != ux_in) HIP_TRY(hipMemcpyAsync(ux_out, ux_in, F, hipMemcpyDeviceToDevice, st));
        if (uy_out != uy_in) HIP_TRY(hipMemcpyAsync(uy_out, uy_in, F, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    HIP_TRY(hipMemcpyAsync(c.u0x, ux_in, F, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.u0y, uy_in, F, hipMemcpyDeviceToDevice, st));
    // targets of stage j: every later stage m (buffer m - 1) and the final sum (buffer nstages - 1).  A target is
    // initialised from u0 at the first stage whose weight on it is nonzero (or, with no nonzero weight, at the stage right
    // before it is read), then accumulated; zero weights are skipped as the reference skips them.
    auto weight = [&](int m, int j) { return m < nstages ? a[m * nstages + j] : b[j]; };
    for (int s = 0; s < steps; ++s) {
        const bool last = s == steps - 1;
        for (int j = 0; j < nstages; ++j) {
            void* tx[MAXT];
            void* ty[MAXT];
            double cw[MAXT];
            int mode[MAXT];
            int count = 0;
            for (int m = j + 1; m <= nstages; ++m) {
                const double w = weight(m, j);
                bool started = false;
                for (int jj = 0; jj < j; ++jj) started = started || weight(m, jj) != 0.0;
                int md = 0;
                if (w != 0.0) md = started ? 2 : 1;
                else if (!started && j == m - 1) md = 3;
                if (!md) continue;
                tx[count] = c.px[m - 1];
                ty[count] = c.py[m - 1];
                cw[count] = w;
                mode[count] = md;
                ++count;
            }
            const void* sx = j == 0 ? c.u0x : c.ucx;
            const void* sy = j == 0 ? c.u0y : c.ucy;
            if ((rc = stage_launch(p, sx, sy, c.u0x, c.u0y, nullptr, nullptr, tx, ty, cw, mode, count, batch, dt, st))) return rc;
            // project the next stage's state (or the final sum)
            const int m = j + 1;
            if ((rc = solve_q(p, c.px[m - 1], c.py[m - 1], batch, c, st))) return rc;
            if (m < nstages) {
                if ((rc = apply_launch(p, c.px[m - 1], c.py[m - 1], c.q, c.ucx, c.ucy, batch, st))) return rc;
            } else {
                void* ox = last ? ux_out : c.u0x;
                void* oy = last ? uy_out : c.u0y;
                if ((rc = apply_launch(p, c.px[m - 1], c.py[m - 1], c.q, ox, oy, batch, st))) return rc;
            }
        }
    }
    return 0;
}

int tcfd_fvm_explicit_terms_vjp(const tcfd_fvm_plan* p, const void* ux, const void* uy, const void* gx, const void* gy,
                                void* out_x, void* out_y, long batch, double dt, void* stream) {
    if (!p || !ux || !uy || !gx || !gy || !out_x || !out_y || batch <= 0)
        return FAIL(TCFD_EINVAL, "fvm_explicit_terms_vjp: bad argument");
    if (p->tangent) return FAIL(TCFD_EINVAL, "fvm_explicit_terms_vjp: a tangent plan (forward over reverse is not provided)");
    if (p->bundle) return FAIL(TCFD_EINVAL, "fvm_explicit_terms_vjp: a bundle plan (forward over reverse is not provided)");
    if (int rce = check_ensemble_batch(p, batch, "fvm_explicit_terms_vjp")) return rce;
    if (out_x == gx || out_x == gy || out_y == gx || out_y == gy || out_x == ux || out_x == uy || out_y == ux || out_y == uy)
        return FAIL(TCFD_EINVAL, "fvm_explicit_terms_vjp: the output may not alias an input (the stencil reads neighbours)");
    return stage_vjp_launch(p, ux, uy, gx, gy, out_x, out_y, 0, batch, dt, (hipStream_t)stream);
}

size_t tcfd_fvm_step_vjp_workspace_bytes(const tcfd_fvm_plan* p, long batch) {
    if (!p || batch <= 0) return 0;
    return carve(p, batch, nullptr, kStepVjp).total;
}

int tcfd_fvm_step_vjp(const tcfd_fvm_plan* p, const void* saved, const void* gx, const void* gy, void* out_x, void* out_y,
                      long batch, int steps, int nstages, const double* a, const double* b, double dt, void* ws, size_t ws_bytes,
                      void* stream) {
    if (!p || !gx || !gy || !out_x || !out_y || batch <= 0 || steps < 0 || (steps > 0 && !saved) || !b || (nstages > 1 && !a))
        return FAIL(TCFD_EINVAL, "fvm_step_vjp: bad argument");
    if (p->tangent) return FAIL(TCFD_EINVAL, "fvm_step_vjp: a tangent plan (forward over reverse is not provided)");
    if (p->bundle) return FAIL(TCFD_EINVAL, "fvm_step_vjp: a bundle plan (forward over reverse is not provided)");
    if (int rce = check_ensemble_batch(p, batch, "fvm_step_vjp")) return rce;
    if (nstages < 1 || nstages > MAXT) return FAIL(TCFD_EINVAL, "fvm_step_vjp: %d stages (1 .. %d supported)", nstages, MAXT);
    for (int i = 0; i < nstages; ++i)
        for (int j = i; j < nstages; ++j)
            if (nstages > 1 && a[i * nstages + j] != 0.0)
                return FAIL(TCFD_EINVAL, "fvm_step_vjp: a[%d][%d] != 0: only explicit (strictly lower) tableaux", i, j);
    int rc = check_ws(p, batch, ws, ws_bytes, kStepVjp);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Carve c = carve(p, batch, ws, kStepVjp);
    const size_t F = field_bytes(p, batch);
    // out holds the running cotangent: that of the result of step s on entry to its reverse, that of its input after
    if (out_x != gx) HIP_TRY(hipMemcpyAsync(out_x, gx, F, hipMemcpyDeviceToDevice, st));
    if (out_y != gy) HIP_TRY(hipMemcpyAsync(out_y, gy, F, hipMemcpyDeviceToDevice, st));
    auto weight = [&](int m, int j) { return m < nstages ? a[m * nstages + j] : b[j]; };
    const int S = nstages;
    for (int s = steps - 1; s >= 0; --s) {
        const char* u0x = (const char*)saved + (size_t)(2 * s) * F;
        const char* u0y = u0x + F;
        // stage states u_1 .. u_{S-1} (u_m in usx[m - 1]) by the forward's stages 0 .. S-2 and targets, the final sum left out
        for (int j = 0; j + 1 < S; ++j) {
            void* tx[MAXT];
            void* ty[MAXT];
            double cw[MAXT];
            int mode[MAXT];
            int count = 0;
            for (int m = j + 1; m < S; ++m) {
                const double w = weight(m, j);
                bool started = false;
                for (int jj = 0; jj < j; ++jj) started = started || weight(m, jj) != 0.0;
                int md = 0;
                if (w != 0.0) md = started ? 2 : 1;
                else if (!started && j == m - 1) md = 3;
                if (!md) continue;
                tx[count] = c.usx[m - 1];
                ty[count] = c.usy[m - 1];
                cw[count] = w;
                mode[count] = md;
                ++count;
            }
            const void* sx = j == 0 ? (const void*)u0x : c.usx[j - 1];
            const void* sy = j == 0 ? (const void*)u0y : c.usy[j - 1];
            if ((rc = stage_launch(p, sx, sy, u0x, u0y, nullptr, nullptr, tx, ty, cw, mode, count, batch, dt, st))) return rc;
            if ((rc = solve_q(p, c.usx[j], c.usy[j], batch, c, st))) return rc;
            if ((rc = apply_launch(p, c.usx[j], c.usy[j], c.q, c.usx[j], c.usy[j], batch, st))) return rc;
        }
        // mu = P u_bar: u_bar = mu, kbar_j = b_j mu
        bool live[MAXT] = {};
        {
            void* tx[MAXA];
            void* ty[MAXA];
            double cw[MAXA];
            int mode[MAXA];
            int count = 0;
            tx[count] = out_x, ty[count] = out_y, cw[count] = 1.0, mode[count++] = 0;
            for (int j = 0; j < S; ++j) {
                if (b[j] == 0.0) continue;
                tx[count] = c.kbx[j], ty[count] = c.kby[j], cw[count] = b[j], mode[count++] = 2;
                live[j] = true;
            }
            if ((rc = solve_q(p, out_x, out_y, batch, c, st))) return rc;
            if ((rc = apply_adj_launch(p, out_x, out_y, c.q, tx, ty, cw, mode, count, batch, st))) return rc;
        }
        for (int i = S - 1; i >= 0; --i) {
            if (!live[i]) continue;   // no weight reads k_i: its cotangent is zero
            if (i == 0) {
                if ((rc = stage_vjp_launch(p, u0x, u0y, c.kbx[0], c.kby[0], out_x, out_y, 1, batch, dt, st))) return rc;
                continue;
            }
            if ((rc = stage_vjp_launch(p, c.usx[i - 1], c.usy[i - 1], c.kbx[i], c.kby[i], c.gbx, c.gby, 0, batch, dt, st)))
                return rc;
            void* tx[MAXA];
            void* ty[MAXA];
            double cw[MAXA];
            int mode[MAXA];
            int count = 0;
            tx[count] = out_x, ty[count] = out_y, cw[count] = 1.0, mode[count++] = 1;
            for (int j = 0; j < i; ++j) {
                const double w = a[i * S + j];
                if (w == 0.0) continue;
                tx[count] = c.kbx[j], ty[count] = c.kby[j], cw[count] = w, mode[count++] = live[j] ? 3 : 2;
                live[j] = true;
            }
            if ((rc = solve_q(p, c.gbx, c.gby, batch, c, st))) return rc;
            if ((rc = apply_adj_launch(p, c.gbx, c.gby, c.q, tx, ty, cw, mode, count, batch, st))) return rc;
        }
    }
    return 0;
}

}  // extern "C"
