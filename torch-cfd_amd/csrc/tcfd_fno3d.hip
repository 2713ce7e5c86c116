// tcfd_fno3d.hip -- MI355X (gfx950) kernels of the FNO3d baseline (fno/fno3d.py:119-236) that the square pointwise family of
// tcfd_fno_pw.hip does not stretch to.  They sit behind the SAME entry points (tcfd_fno_pointwise_pre, tcfd_fno_pointwise_bwd_out:
// pw_dispatch / pointwise_bwd_impl of tcfd_fno_pw.hip end in the two dispatch functions at the bottom of this file):
//
//   * the lifting  p : (b, ci, P) -> (b, W, P),  one 1x1x1 convolution with ci = input_channel + 3 (13 in the notebook) != W.
//       forward   k_pw_rect_in<W, V>    a lane owns V consecutive points and W accumulators; the input channels are streamed through
//                                        (ci is a trip count, not a template parameter), the weight row of a channel is lane uniform
//       dW, db    k_rect_wgrad<TO, TI>  sums over all points of outer products dout (x) [x, 1]: a GEMM whose K axis is the points.
//                                        Lane (q, c) loads the 16-byte runs dout[c][4q..4q+3] and x[c][4q..4q+3]; register r of the two
//                                        runs IS the A resp. B fragment of the k-step over the points {4q + r} of
//                                        v_mfma_f32_16x16x4_f32 (the layout of k_sample_outer_mfma), so a group of 16 points costs
//                                        4 TO TI matrix instructions and nothing else.  Per-wave partial sums, added by the caller
//                                        (tcfd_sum_rows_scatter: deterministic, no atomics).
//       dx        k_rect_dx<W, V>       only when the network input itself requires a gradient: W cotangents in registers, the ci
//                                        input channels streamed out
//     All three move each activation once and do 2 ci W flop per point on 4 (ci + W) bytes (5.7 flop/B at 13 -> 10): bandwidth bound.
//
//   * the head  q = mlp2(GELU(mlp1(v))) : W -> E -> 1  (last_activation=True), forward.  k_head_fwd<W, V>: the channels of a point in
//     registers, the E hidden units one after the other (E is a trip count), ONE accumulator: 2 E (W + 1) flop + E GELUs per point
//     on 4 (W + 1) bytes, ~64 flop/B at W = 10 -- bound by the vector unit (packed multiply-adds + the 10-instruction packed GELU of
//     tcfd_fno_pw.hpp), not by memory.  The (b, E, P) hidden tensor never exists.  Its backward is the tiled matrix-pipe kernel
//     (tcfd_fno_tiles.hip).  With the identity between the two layers the head folds into ONE W -> 1 reduction on the host
//     (fno.py) and needs no kernel of its own.
//
// Alignment rules of the family: 16-byte (8-byte) accesses when P % 4 (P % 2) == 0 and the base pointers are aligned, else one
// point per lane / guarded 4-byte loads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "tcfd_fno_common.hpp"
#include "tcfd_fno_pw.hpp"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

template <int V> struct RectVec { typedef float type; };
template <> struct RectVec<2> { typedef v2f type; };
template <> struct RectVec<4> { typedef f4 type; };

__device__ __forceinline__ float rect_fma(float w, float x, float acc) { return fmaf(w, x, acc); }
__device__ __forceinline__ v2f rect_fma(float w, v2f x, v2f acc) { return __builtin_elementwise_fma(v2f{w, w}, x, acc); }
__device__ __forceinline__ f4 rect_fma(float w, f4 x, f4 acc) { return __builtin_elementwise_fma(f4{w, w, w, w}, x, acc); }
__device__ __forceinline__ float rect_act(float v, int act) { return pw_act(v, act); }
__device__ __forceinline__ v2f rect_act(v2f v, int act) { return pw_act(v, act); }
__device__ __forceinline__ f4 rect_act(f4 v, int act) {
    const v2f lo = pw_act(v2f{v.x, v.y}, act), hi = pw_act(v2f{v.z, v.w}, act);
    return f4{lo.x, lo.y, hi.x, hi.y};
}

// out[o] = act2( b2[o] + sum_i w2t[i][o] x[i] ),  o < CO, i < ci
template <int CO, int V>
__global__ __launch_bounds__(256) void k_pw_rect_in(PwArgs a, int ci) {
    typedef typename RectVec<V>::type vf;
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const int b = blockIdx.y;
    if (p >= a.P) return;                       // V > 1: P % V == 0 (host), a lane's points are all inside
    vf o[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) o[c] = (vf)(a.b2 ? a.b2[c] : 0.f);
    const float* xb = a.x + (size_t)b * ci * a.P + p;
#pragma unroll 4
    for (int i = 0; i < ci; ++i) {
        const vf xv = PW_LOAD(reinterpret_cast<const vf*>(xb + (size_t)i * a.P));
        const float* w = a.w2t + i * CO;
#pragma unroll
        for (int c = 0; c < CO; ++c) o[c] = rect_fma(w[c], xv, o[c]);
    }
    float* ob = a.out + (size_t)b * CO * a.P + p;
    if (a.pre) {
        float* zb = a.pre + (size_t)b * CO * a.P + p;
#pragma unroll
        for (int c = 0; c < CO; ++c) __builtin_nontemporal_store(o[c], reinterpret_cast<vf*>(zb + (size_t)c * a.P));
    }
#pragma unroll
    for (int c = 0; c < CO; ++c) __builtin_nontemporal_store(rect_act(o[c], a.act2), reinterpret_cast<vf*>(ob + (size_t)c * a.P));
}

// dx[i] = sum_o w2t[i][o] dout[o],  i < ci  (the single layer without an output activation)
template <int CO, int V>
__global__ __launch_bounds__(256) void k_rect_dx(PwBwdArgs a, int ci) {
    typedef typename RectVec<V>::type vf;
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const int b = blockIdx.y;
    if (p >= a.P) return;
    vf g[CO];
    const float* gb = a.dout + (size_t)b * CO * a.P + p;
#pragma unroll
    for (int c = 0; c < CO; ++c) g[c] = PW_LOAD(reinterpret_cast<const vf*>(gb + (size_t)c * a.P));
    float* db = a.dx + (size_t)b * ci * a.P + p;
    for (int i = 0; i < ci; ++i) {
        const float* w = a.w2t + i * CO;
        vf s = (vf)(0.f);
#pragma unroll
        for (int c = 0; c < CO; ++c) s = rect_fma(w[c], g[c], s);
        __builtin_nontemporal_store(s, reinterpret_cast<vf*>(db + (size_t)i * a.P));
    }
}

// four consecutive values of a channel row of P floats starting at point p: one 16-byte load (vec: P % 4 == 0 and an aligned
// base, so the run is all inside or all outside), else guarded 4-byte loads; 0 beyond P
__device__ __forceinline__ f4 rect_load4(const float* row, long p, long P, bool vec) {
    if (vec) return p < P ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(row + p)) : f4{0.f, 0.f, 0.f, 0.f};
    f4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p + k < P ? row[p + k] : 0.f;
    return v;
}

// partials[wave][o][i] = sum over the wave's points of dout[o] x[i]  (i < ci),  [o][ci] = sum of dout[o]; rows of 16 TO x 16 TI
template <int TO, int TI>
__global__ __launch_bounds__(256) void k_rect_wgrad(PwBwdArgs a, int ci, int co, int vec, long gpb, long total) {
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
    const long wid = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (long)gridDim.x * 4;
    f4 acc[TO][TI];
#pragma unroll
    for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) acc[to][ti] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long G = wid; G < total; G += nw) {
        const long b = G / gpb;
        const long p = (G - b * gpb) * 16 + 4 * q;
        f4 g[TO], v[TI];
#pragma unroll
        for (int to = 0; to < TO; ++to) {
            const int o = 16 * to + c;
            g[to] = rect_load4(a.dout + ((size_t)b * co + (o < co ? o : 0)) * a.P, p, a.P, vec != 0);
            if (o >= co) g[to] = f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) {
            const int ch = 16 * ti + c;
            if (16 * ti < ci) v[ti] = rect_load4(a.x + ((size_t)b * ci + (ch < ci ? ch : 0)) * a.P, p, a.P, vec != 0);
            if (ch >= ci) { const float ones = ch == ci ? 1.f : 0.f; v[ti] = f4{ones, ones, ones, ones}; }     // (dout is 0 beyond P)
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int to = 0; to < TO; ++to)
#pragma unroll
                for (int ti = 0; ti < TI; ++ti) acc[to][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[to][r], v[ti][r], acc[to][ti], 0, 0, 0);
    }
    float* out = a.partials + (size_t)wid * (256 * TO * TI);
#pragma unroll
    for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int ti = 0; ti < TI; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(16 * to + 4 * q + r) * (16 * TI) + 16 * ti + c] = acc[to][ti][r];
}

// out = act2( b2 + sum_m w2[m] act1( b1[m] + sum_i w1[m][i] x[i] ) ): the per-point arithmetic is pw_core's (tcfd_fno_pw.hpp)
template <int CI, int V>
__global__ __launch_bounds__(256) void k_head_fwd(PwArgs a) {
    typedef typename PwVec<V>::type vf;
    const long p = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const int b = blockIdx.y;
    if (p >= a.P) return;
    vf x[CI], o[1];
    const float* xb = a.x + (size_t)b * CI * a.P + p;
#pragma unroll
    for (int i = 0; i < CI; ++i) x[i] = PW_LOAD(reinterpret_cast<const vf*>(xb + (size_t)i * a.P));
    pw_core<CI, 0, 1, true, vf>(a, b, x, o);
    float* ob = a.out + (size_t)b * a.P + p;
    if (a.pre) __builtin_nontemporal_store(o[0], reinterpret_cast<vf*>(a.pre + (size_t)b * a.P + p));
    __builtin_nontemporal_store(pw_act(o[0], a.act2), reinterpret_cast<vf*>(ob));
}

template <typename... Ptr>
bool aligned_to(size_t bytes, Ptr... ptrs) { return ((... | (uintptr_t)ptrs) % bytes) == 0; }

template <int CO>
int launch_rect_in(const PwArgs& a, int batch, int ci, hipStream_t st) {
    FnoProfScope prof(FNO_K_POINTWISE_1, st);
    // four points per lane up to width 16, two above (4 W accumulators: 128 registers at width 32 would halve the waves in flight
    // of a kernel that lives on memory-level parallelism)
    constexpr int V = CO <= 16 ? 4 : 2;
    if (a.P % V == 0 && aligned_to(4 * V, a.x, a.out, a.pre)) {
        hipLaunchKernelGGL((k_pw_rect_in<CO, V>), dim3((unsigned)((a.P / V + 255) / 256), (unsigned)batch), dim3(256), 0, st, a, ci);
    } else {
        hipLaunchKernelGGL((k_pw_rect_in<CO, 1>), dim3((unsigned)((a.P + 255) / 256), (unsigned)batch), dim3(256), 0, st, a, ci);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int CI>
int launch_head_fwd(const PwArgs& a, int batch, hipStream_t st) {
    FnoProfScope prof(FNO_K_POINTWISE, st);
    if (a.P % 2 == 0 && aligned_to(8, a.x, a.out, a.pre)) {
        hipLaunchKernelGGL((k_head_fwd<CI, 2>), dim3((unsigned)((a.P / 2 + 255) / 256), (unsigned)batch), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_head_fwd<CI, 1>), dim3((unsigned)((a.P + 255) / 256), (unsigned)batch), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int CO>
int launch_rect_dx(const PwBwdArgs& a, int batch, int ci, hipStream_t st) {
    constexpr int V = CO <= 16 ? 4 : 2;
    if (a.P % V == 0 && aligned_to(4 * V, a.dout, a.dx)) {
        hipLaunchKernelGGL((k_rect_dx<CO, V>), dim3((unsigned)((a.P / V + 255) / 256), (unsigned)batch), dim3(256), 0, st, a, ci);
    } else {
        hipLaunchKernelGGL((k_rect_dx<CO, 1>), dim3((unsigned)((a.P + 255) / 256), (unsigned)batch), dim3(256), 0, st, a, ci);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int TO, int TI>
int launch_rect_wgrad(const PwBwdArgs& a, int batch, int ci, int co, int max_waves, int* dims, hipStream_t st) {
    const long gpb = (a.P + 15) / 16, total = gpb * batch;
    // <= 8 waves per SIMD's worth of rows (256 CUs x 4 SIMDs x 8 / 4 waves per workgroup)
    long blocks = std::min<long>({(total + 3) / 4, (long)(max_waves / 4), 2048L});
    if (blocks < 1) blocks = 1;
    const int vec = (a.P % 4 == 0 && aligned_to(16, a.x, a.dout)) ? 1 : 0;
    hipLaunchKernelGGL((k_rect_wgrad<TO, TI>), dim3((unsigned)blocks), dim3(256), 0, st, a, ci, co, vec, gpb, total);
    HIP_TRY(hipGetLastError());
    dims[5] = (int)(blocks * 4);
    return 0;
}

}  // namespace

// Forward shapes of the FNO3d baseline behind tcfd_fno_pointwise_pre (called by pw_dispatch after its own cases; *handled = 0:
// not covered).  Single layer ci -> W with ci in [1, 64] and W an even width 4 ... 32; two layers W -> E -> 1 with any E.
int tcfd_pw_fno3d_dispatch(const PwArgs& a, int batch, int ci, int cm, int co, hipStream_t st, int* handled) {
    *handled = 0;
    if (a.pe || a.frame || a.skip_mode != 0 || a.w2_bstride || a.b2_bstride) return 0;
    if (!a.w1) {
        if (ci < 1 || ci > 64) return 0;
#define RECT_IN(W_) if (co == W_) { *handled = 1; return launch_rect_in<W_>(a, batch, ci, st); }
        RECT_IN(4) RECT_IN(6) RECT_IN(8) RECT_IN(10) RECT_IN(12) RECT_IN(14) RECT_IN(16) RECT_IN(18) RECT_IN(20) RECT_IN(22)
        RECT_IN(24) RECT_IN(26) RECT_IN(28) RECT_IN(30) RECT_IN(32)
#undef RECT_IN
        return 0;
    }
    if (co != 1 || cm < 1) return 0;
#define HEAD_FWD(W_) if (ci == W_) { *handled = 1; return launch_head_fwd<W_>(a, batch, st); }
    HEAD_FWD(4) HEAD_FWD(6) HEAD_FWD(8) HEAD_FWD(10) HEAD_FWD(12) HEAD_FWD(14) HEAD_FWD(16) HEAD_FWD(18) HEAD_FWD(20) HEAD_FWD(22)
    HEAD_FWD(24) HEAD_FWD(26) HEAD_FWD(28) HEAD_FWD(30) HEAD_FWD(32)
#undef HEAD_FWD
    return 0;
}

// Backward of the single layer ci -> W without an output activation behind tcfd_fno_pointwise_bwd[_out] (called by
// pointwise_bwd_impl after its own cases).  Row layout reported in dims: A (16 TO x 16 TI) = [dW | db] with db in column ci, no B
// part; a.x == NULL: layout query.
int tcfd_pwb_rect_dispatch(const PwBwdArgs& a, int batch, int ci, int co, int max_waves, int* dims, hipStream_t st, int* handled) {
    *handled = 0;
    if (a.pe || a.per_sample || a.skip_mode != 0 || a.act2 != 0 || ci < 1 || ci > 64 || co < 4 || co > 32 || (co & 1)) return 0;
    *handled = 1;
    const int to = (co + 15) / 16, ti = (ci + 16) / 16;
    dims[0] = 16 * to; dims[1] = 16 * ti; dims[2] = 0; dims[3] = 0; dims[4] = 256 * to * ti; dims[5] = 0;
    if (!a.x) return 0;
    if (max_waves < 4) return FAIL(TCFD_EINVAL, "fno_pointwise_bwd: %d rows of partial sums given, 4 needed", max_waves);
    FnoProfScope prof(FNO_K_POINTWISE_BWD_1, st);
    if (a.dx) {
        int rc = -1;
#define RECT_DX(W_) if (co == W_) rc = launch_rect_dx<W_>(a, batch, ci, st);
        RECT_DX(4) RECT_DX(6) RECT_DX(8) RECT_DX(10) RECT_DX(12) RECT_DX(14) RECT_DX(16) RECT_DX(18) RECT_DX(20) RECT_DX(22)
        RECT_DX(24) RECT_DX(26) RECT_DX(28) RECT_DX(30) RECT_DX(32)
#undef RECT_DX
        if (rc) return rc;
    }
#define RECT_WG(TO_, TI_) if (to == TO_ && ti == TI_) return launch_rect_wgrad<TO_, TI_>(a, batch, ci, co, max_waves, dims, st);
    RECT_WG(1, 1) RECT_WG(1, 2) RECT_WG(1, 3) RECT_WG(1, 4) RECT_WG(1, 5) RECT_WG(2, 1) RECT_WG(2, 2) RECT_WG(2, 3) RECT_WG(2, 4)
    RECT_WG(2, 5)
#undef RECT_WG
    return FAIL(TCFD_EINVAL, "fno_pointwise_bwd: channels (%d -> %d) not instantiated", ci, co);
}
