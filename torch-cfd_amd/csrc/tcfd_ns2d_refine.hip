// tcfd_ns2d_refine.hip -- the spectral refiner of the fine-tuning head, on the solver plan's sweeps: its elementwise kernels, its
// scratch layout and its three entry points.  The explicit-terms sweep and its VJP are reached through the C ABI and
// ns2d::explicit_chunked, the transforms through the sized units (tcfd_ns2d_plan.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tcfd_ns2d_plan.hpp"

using namespace tcfd;

// ------------------------------------------------------------------ spectral refiner (fno/finetune.py::OutConvFT._fine_tune)
// Real time-last trajectories w (batch, n, n, nt) -> (w, w_t, residual) of the weighted Crank-Nicolson pair at -dt / +dt and
// the residual of the weighted state, all time-last, in one call.  Per (sample, step) slice, with C(.) = mask . rfft2(u.grad)
// and L the plan's linear term (here: the reference's Laplacian table with L(0,0) = 1):
//     wh = rfft2(w);  C1 = C(wh)
//     wn(d) = (-d C1 + d f + (1 + 0.5 d nu L) wh) / (1 - 0.5 d nu L),   wt(d) = (wn(d) - wh) / d      (d = -dt, +dt)
//     W = a wn(-dt) + b wn(dt),  Wt = a wt(-dt) + b wt(dt),   R = Wt + C(W) - nu L W - f
// in the reference's operation order.  C is the plan's explicit-terms sweep (column pass, fused row pass, column pass; F = -C:
// the plan carries no forcing).  The VJP recomputes wh and W and runs the explicit-terms VJP row pass for both convections.
template <typename T>
__global__ __launch_bounds__(256) void k_refine_transpose(const T* __restrict__ in, T* __restrict__ out, long total, long plane,
                                                          int nt, int to_time_first) {
    // time-first index e = (s nt + t) plane + i  <->  time-last index (s plane + i) nt + t
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        if (to_time_first) {
            const long i = e % plane, st = e / plane, t = st % nt, s = st / nt;
            out[e] = in[(s * plane + i) * nt + t];
        } else {     // e runs over the time-last output: coalesced stores
            const long t = e % nt, si = e / nt, i = si % plane, s = si / plane;
            out[e] = in[(s * nt + t) * plane + i];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_refine_cn(const cx<T>* __restrict__ wh, const cx<T>* __restrict__ F1,
                                                   const cx<T>* __restrict__ fh, const T* __restrict__ Lt, cx<T>* __restrict__ W,
                                                   cx<T>* __restrict__ Wt, long total, long plane, int nt, T dt, T visc, T ca,
                                                   T cb) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long p = e % plane;
        const T L = Lt[p];
        const cx<T> w = wh[e];
        const cx<T> C = mk<T>(-F1[e].x, -F1[e].y);
        const cx<T> f = fh ? fh[(e / (plane * nt)) * plane + p] : mk<T>((T)0, (T)0);
        cx<T> wn[2], wt[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const T d = k ? dt : -dt;
            const T hl = (((T)0.5 * d) * visc) * L;
            cx<T> num = cscale(C, -d);
            if (fh) num = num + cscale(f, d);
            num = num + cscale(w, (T)1 + hl);
            const T den = (T)1 - hl;
            wn[k] = mk<T>(num.x / den, num.y / den);
            const cx<T> dw = wn[k] - w;
            wt[k] = mk<T>(dw.x / d, dw.y / d);
        }
        W[e] = cscale(wn[0], ca) + cscale(wn[1], cb);
        Wt[e] = cscale(wt[0], ca) + cscale(wt[1], cb);
    }
}

// R = Wt + C2 - nu L W - f, C2 = -F2; written over F2
template <typename T>
__global__ __launch_bounds__(256) void k_refine_res(const cx<T>* __restrict__ W, const cx<T>* __restrict__ Wt, cx<T>* F2R,
                                                    const cx<T>* __restrict__ fh, const T* __restrict__ Lt, long total, long plane,
                                                    int nt, T visc) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long p = e % plane;
        const T vl = visc * Lt[p];
        const cx<T> C = mk<T>(-F2R[e].x, -F2R[e].y);
        cx<T> r = (Wt[e] + C) - cscale(W[e], vl);
        if (fh) r = r - fh[(e / (plane * nt)) * plane + p];
        F2R[e] = r;
    }
}

// the closing sum of the explicit-terms VJP, sum_f post_f X_f with post_f = -(c / n^2) conj(a_f), from the plan's 1-D tables
template <typename T>
__device__ __forceinline__ cx<T> refine_vjp_sum(const cx<T>* __restrict__ X, long e, long total, T kx, T ky, T c, int n) {
    const T two_pi = (T)(2.0 * 3.14159265358979323846);
    T lap = (T)(-4.0 * 3.14159265358979323846 * 3.14159265358979323846) * (kx * kx + ky * ky);
    if (kx == (T)0 && ky == (T)0) lap = (T)1;
    // a_f = i s_f with real s_f:  s = (-2 pi ky / lap, 2 pi kx / lap, 2 pi kx, 2 pi ky);  conj(a_f) x = -i s_f x
    const T s[4] = {-two_pi * ky / lap, two_pi * kx / lap, two_pi * kx, two_pi * ky};
    cx<T> acc = mk<T>((T)0, (T)0);
#pragma unroll
    for (int f = 0; f < 4; ++f) acc = acc + cscale(mul_mi(X[(long)f * total + e]), s[f]);
    return cscale(acc, -c / ((T)n * (T)n));
}

template <typename T>
__device__ __forceinline__ T col_weight(long p, int m) {
    const long j = p % m;
    return (j == 0 || j == m - 1) ? (T)1 : (T)2;
}

// cotangents of the outputs (raw rfft2 of the time-first real cotangents) -> the residual's share:
//   gR = sc GR, gWt = sc GWt + gR, gW = sc GW - nu L gR, gm2 = -gR mask / c     (sc = c / n^2: the adjoint of the c2r transform)
template <typename T>
__global__ __launch_bounds__(256) void k_refine_vjp_out(cx<T>* GW, cx<T>* GWt, cx<T>* GR, cx<T>* __restrict__ gm2,
                                                        const T* __restrict__ Lt, const T* __restrict__ Mt, long total, long plane,
                                                        int n, int m, T visc, int has_w, int has_wt, int has_r) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long p = e % plane;
        const T c = col_weight<T>(p, m), sc = c / ((T)n * (T)n);
        const cx<T> z = mk<T>((T)0, (T)0);
        const cx<T> gR = has_r ? cscale(GR[e], sc) : z;
        const cx<T> gWt = (has_wt ? cscale(GWt[e], sc) : z) + gR;
        const cx<T> gW = (has_w ? cscale(GW[e], sc) : z) - cscale(gR, visc * Lt[p]);
        GW[e] = gW;
        GWt[e] = gWt;
        GR[e] = gR;
        gm2[e] = cscale(gR, -Mt[p] / c);
    }
}

// the Crank-Nicolson pair and the weighting, backwards: gW += VJP of C(W); then per d the shares of wh, C1 and f.
// Writes the wh cotangent (partial) over GW, the forcing share over GR and gm1 = -gC1 mask / c over gm.
template <typename T>
__global__ __launch_bounds__(256) void k_refine_vjp_cn(cx<T>* GW, const cx<T>* __restrict__ GWt, cx<T>* GR, cx<T>* gm,
                                                       const cx<T>* __restrict__ X, const T* __restrict__ Lt,
                                                       const T* __restrict__ Mt, const T* __restrict__ kx, const T* __restrict__ ky,
                                                       long total, long plane, int n, int m, T dt, T visc, T ca, T cb) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long p = e % plane;
        const T c = col_weight<T>(p, m), L = Lt[p];
        const cx<T> gW = GW[e] + refine_vjp_sum<T>(X, e, total, kx[p / m], ky[p % m], c, n);
        const cx<T> gWt = GWt[e];
        cx<T> gwh = mk<T>((T)0, (T)0), gC1 = gwh, gf = mk<T>(-GR[e].x, -GR[e].y);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const T d = k ? dt : -dt, co = k ? cb : ca;
            const T hl = (((T)0.5 * d) * visc) * L, r = (T)1 / ((T)1 - hl);
            const cx<T> gwt = cscale(gWt, co / d);                 // share of wt(d), divided by d
            const cx<T> gwn = cscale(gW, co) + gwt;
            gwh = gwh - gwt + cscale(gwn, ((T)1 + hl) * r);
            gC1 = gC1 - cscale(gwn, d * r);
            gf = gf + cscale(gwn, d * r);
        }
        GW[e] = gwh;
        GR[e] = gf;
        gm[e] = cscale(gC1, -Mt[p] / c);                          // C1 = -F1: gm1 = g_F1 mask / c = -g_C1 mask / c
    }
}

// g_wh (partial + VJP of C(wh)) -> n^2 g / c, the input of the c2r transform that is the adjoint of rfft2
template <typename T>
__global__ __launch_bounds__(256) void k_refine_vjp_in(cx<T>* GW, const cx<T>* __restrict__ X, const T* __restrict__ kx,
                                                       const T* __restrict__ ky, long total, long plane, int n, int m) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long p = e % plane;
        const T c = col_weight<T>(p, m);
        const cx<T> g = GW[e] + refine_vjp_sum<T>(X, e, total, kx[p / m], ky[p % m], c, n);
        GW[e] = cscale(g, (T)n * (T)n / c);
    }
}

// gf[s] = sum_t G[s, t]: the forcing half spectrum is shared by the nt steps of a sample
template <typename T>
__global__ __launch_bounds__(256) void k_refine_sum_t(const cx<T>* __restrict__ G, cx<T>* __restrict__ gf, long total, long plane,
                                                      int nt) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long p = e % plane, s = e / plane;
        cx<T> acc = mk<T>((T)0, (T)0);
        for (int t = 0; t < nt; ++t) acc = acc + G[(s * nt + t) * plane + p];
        gf[e] = acc;
    }
}

static unsigned refine_blocks(long total) { return (unsigned)std::min<long>((total + 255) / 256, 1 << 16); }

struct RefineWs {
    unsigned char* r0;      // time-first real scratch (bt n n)
    unsigned char* cf[10];  // complex fields (bt n m)
    unsigned char* ex;      // workspace of the explicit-terms / transform sweeps
    size_t ex_bytes;
};
static size_t refine_real_bytes(const tcfd_ns2d_plan* p, long bt) {
    return align256((size_t)bt * p->n * p->n * (p->dtype == TCFD_C128 ? 8 : 4));
}
static size_t refine_cx_bytes(const tcfd_ns2d_plan* p, long bt) {
    return align256((size_t)bt * p->n * p->m * (p->dtype == TCFD_C128 ? 16 : 8));
}
static RefineWs refine_carve(const tcfd_ns2d_plan* p, void* ws, long bt) {
    RefineWs r;
    unsigned char* b = (unsigned char*)ws;
    r.r0 = b;
    b += refine_real_bytes(p, bt);
    for (int k = 0; k < 10; ++k) { r.cf[k] = b; b += refine_cx_bytes(p, bt); }
    r.ex = b;
    r.ex_bytes = tcfd_ns2d_workspace_bytes(p, bt);
    return r;
}

template <typename T>
static int refine_transpose(const void* in, void* out, long batch, int nt, long plane, int to_tf, hipStream_t st) {
    const long total = batch * nt * plane;
    hipLaunchKernelGGL(k_refine_transpose<T>, dim3(refine_blocks(total)), dim3(256), 0, st, (const T*)in, (T*)out, total, plane,
                       nt, to_tf);
    HIP_TRY(hipGetLastError());
    return 0;
}

// time-last real x -> half spectra (bt, n, m)
template <typename T>
static int refine_rfft_tl(const tcfd_ns2d_plan* p, const void* x, void* xh, long batch, int nt, const RefineWs& R, hipStream_t st) {
    int rc;
    if ((rc = refine_transpose<T>(x, R.r0, batch, nt, (long)p->n * p->n, 1, st))) return rc;
    return ns2d::rfft2<T>(p, R.r0, xh, batch * nt, st);
}
// half spectra -> time-last real
template <typename T>
static int refine_irfft_tl(const tcfd_ns2d_plan* p, const void* xh, void* x, long batch, int nt, const RefineWs& R, hipStream_t st) {
    int rc;
    if ((rc = ns2d::irfft2<T>(p, xh, R.r0, batch * nt, R.ex, st))) return rc;
    return refine_transpose<T>(R.r0, x, batch, nt, (long)p->n * p->n, 0, st);
}

template <typename T>
static int refine_forward_state(const tcfd_ns2d_plan* p, const void* w, const void* fh, void* wh, void* F, void* W, void* Wt,
                                long batch, int nt, double dt, double visc, double ca, double cb, const RefineWs& R, hipStream_t st) {
    const long bt = batch * nt, plane = (long)p->n * p->m, total = bt * plane;
    int rc;
    if ((rc = refine_rfft_tl<T>(p, w, wh, batch, nt, R, st))) return rc;
    if ((rc = ns2d::explicit_chunked(p, wh, F, nullptr, nullptr, false, bt, R.ex, st))) return rc;
    hipLaunchKernelGGL(k_refine_cn<T>, dim3(refine_blocks(total)), dim3(256), 0, st, (const cx<T>*)wh, (const cx<T>*)F,
                       (const cx<T>*)fh, (const T*)p->lin, (cx<T>*)W, (cx<T>*)Wt, total, plane, nt, (T)dt, (T)visc, (T)ca, (T)cb);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
static int refine_impl(const tcfd_ns2d_plan* p, const void* w, const void* fh, void* w_out, void* wt_out, void* res_out,
                       long batch, int nt, double dt, double visc, double ca, double cb, void* ws, hipStream_t st) {
    const long bt = batch * nt, plane = (long)p->n * p->m, total = bt * plane;
    const RefineWs R = refine_carve(p, ws, bt);
    void *wh = R.cf[0], *F = R.cf[1], *W = R.cf[2], *Wt = R.cf[3];
    int rc;
    if ((rc = refine_forward_state<T>(p, w, fh, wh, F, W, Wt, batch, nt, dt, visc, ca, cb, R, st))) return rc;
    if (res_out) {
        if ((rc = ns2d::explicit_chunked(p, W, F, nullptr, nullptr, false, bt, R.ex, st))) return rc;
        hipLaunchKernelGGL(k_refine_res<T>, dim3(refine_blocks(total)), dim3(256), 0, st, (const cx<T>*)W, (const cx<T>*)Wt,
                           (cx<T>*)F, (const cx<T>*)fh, (const T*)p->lin, total, plane, nt, (T)visc);
        HIP_TRY(hipGetLastError());
        if ((rc = refine_irfft_tl<T>(p, F, res_out, batch, nt, R, st))) return rc;
    }
    if (w_out && (rc = refine_irfft_tl<T>(p, W, w_out, batch, nt, R, st))) return rc;
    if (wt_out && (rc = refine_irfft_tl<T>(p, Wt, wt_out, batch, nt, R, st))) return rc;
    return 0;
}

template <typename T>
static int refine_vjp_impl(const tcfd_ns2d_plan* p, const void* w, const void* fh, const void* g_w, const void* g_wt,
                           const void* g_res, void* grad_w, void* grad_fh, long batch, int nt, double dt, double visc, double ca,
                           double cb, void* ws, hipStream_t st) {
    const long bt = batch * nt, plane = (long)p->n * p->m, total = bt * plane;
    const RefineWs R = refine_carve(p, ws, bt);
    void *wh = R.cf[0], *W = R.cf[1], *GW = R.cf[2], *GWt = R.cf[3], *GR = R.cf[4], *M = R.cf[5], *X = R.cf[6];
    const size_t ex_need = tcfd_ns2d_workspace_bytes(p, bt);
    int rc;
    // forward state: wh, W (F1 in M, Wt in GWt -- both dead before their slots are reused)
    if ((rc = refine_forward_state<T>(p, w, fh, wh, M, W, GWt, batch, nt, dt, visc, ca, cb, R, st))) return rc;
    if (g_w && (rc = refine_rfft_tl<T>(p, g_w, GW, batch, nt, R, st))) return rc;
    if (g_wt && (rc = refine_rfft_tl<T>(p, g_wt, GWt, batch, nt, R, st))) return rc;
    if (g_res && (rc = refine_rfft_tl<T>(p, g_res, GR, batch, nt, R, st))) return rc;
    hipLaunchKernelGGL(k_refine_vjp_out<T>, dim3(refine_blocks(total)), dim3(256), 0, st, (cx<T>*)GW, (cx<T>*)GWt, (cx<T>*)GR,
                       (cx<T>*)M, (const T*)p->lin, (const T*)p->mask, total, plane, p->n, p->m, (T)visc, g_w ? 1 : 0,
                       g_wt ? 1 : 0, g_res ? 1 : 0);
    HIP_TRY(hipGetLastError());
    // the convection of the weighted state
    if ((rc = tcfd_ns2d_explicit_terms_vjp(p, W, M, X, bt, R.ex, ex_need, st))) return rc;
    hipLaunchKernelGGL(k_refine_vjp_cn<T>, dim3(refine_blocks(total)), dim3(256), 0, st, (cx<T>*)GW, (const cx<T>*)GWt, (cx<T>*)GR,
                       (cx<T>*)M, (const cx<T>*)X, (const T*)p->lin, (const T*)p->mask, (const T*)p->kx, (const T*)p->ky, total,
                       plane, p->n, p->m, (T)dt, (T)visc, (T)ca, (T)cb);
    HIP_TRY(hipGetLastError());
    // the convection of the input state
    if ((rc = tcfd_ns2d_explicit_terms_vjp(p, wh, M, X, bt, R.ex, ex_need, st))) return rc;
    hipLaunchKernelGGL(k_refine_vjp_in<T>, dim3(refine_blocks(total)), dim3(256), 0, st, (cx<T>*)GW, (const cx<T>*)X,
                       (const T*)p->kx, (const T*)p->ky, total, plane, p->n, p->m);
    HIP_TRY(hipGetLastError());
    if (grad_w && (rc = refine_irfft_tl<T>(p, GW, grad_w, batch, nt, R, st))) return rc;
    if (grad_fh) {
        const long tf = batch * plane;
        hipLaunchKernelGGL(k_refine_sum_t<T>, dim3(refine_blocks(tf)), dim3(256), 0, st, (const cx<T>*)GR, (cx<T>*)grad_fh, tf, plane,
                           nt);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" size_t tcfd_ns2d_refine_workspace_bytes(const tcfd_ns2d_plan* p, long batch, int nt) {
    if (!p || batch <= 0 || nt <= 0) return 0;
    const long bt = batch * nt;
    return refine_real_bytes(p, bt) + 10 * refine_cx_bytes(p, bt) + tcfd_ns2d_workspace_bytes(p, bt);
}

extern "C" int tcfd_ns2d_refine(const tcfd_ns2d_plan* p, const void* w, const void* f_hat, void* w_out, void* wt_out,
                              void* res_out, long batch, int nt, double dt, double visc, double bdf0, double bdf1, void* ws,
                              size_t ws_bytes, void* stream) {
    if (!p || !w || batch <= 0 || nt <= 0 || dt == 0.0) return fail(TCFD_EINVAL, "refine: bad argument");
    if (p->ens_count > 0)
        return fail(TCFD_EINVAL, "refine: not implemented for a plan with per-sample parameters (tcfd_ns2d_plan_set_ensemble): the "
                    "refiner reads one linear-term table");
    if (int rc_ = check_batch(p, batch * nt)) return rc_;   // every (sample, step) slice is one field of the sweeps
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_refine_workspace_bytes(p, batch, nt));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->dtype == TCFD_C128)
        return refine_impl<double>(p, w, f_hat, w_out, wt_out, res_out, batch, nt, dt, visc, bdf0, bdf1, ws, st);
    return refine_impl<float>(p, w, f_hat, w_out, wt_out, res_out, batch, nt, dt, visc, bdf0, bdf1, ws, st);
}

extern "C" int tcfd_ns2d_refine_vjp(const tcfd_ns2d_plan* p, const void* w, const void* f_hat, const void* g_w, const void* g_wt,
                                  const void* g_res, void* grad_w, void* grad_f_hat, long batch, int nt, double dt, double visc,
                                  double bdf0, double bdf1, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || batch <= 0 || nt <= 0 || dt == 0.0) return fail(TCFD_EINVAL, "refine_vjp: bad argument");
    if (p->ens_count > 0)
        return fail(TCFD_EINVAL, "refine_vjp: not implemented for a plan with per-sample parameters (tcfd_ns2d_plan_set_ensemble): the "
                    "refiner reads one linear-term table");
    if (grad_f_hat && !f_hat) return fail(TCFD_EINVAL, "refine_vjp: grad_f_hat needs f_hat");
    if (int rc_ = check_batch(p, batch * nt)) return rc_;
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_refine_workspace_bytes(p, batch, nt));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->dtype == TCFD_C128)
        return refine_vjp_impl<double>(p, w, f_hat, g_w, g_wt, g_res, grad_w, grad_f_hat, batch, nt, dt, visc, bdf0, bdf1, ws, st);
    return refine_vjp_impl<float>(p, w, f_hat, g_w, g_wt, g_res, grad_w, grad_f_hat, batch, nt, dt, visc, bdf0, bdf1, ws, st);
}
