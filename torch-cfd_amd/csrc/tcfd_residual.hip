// tcfd_residual.hip -- MI355X (gfx950) kernels + C ABI for the losses of fno/losses.py other than SobolevLoss:
//   * the physics-informed residual of the vorticity equation over a predicted space-time block (ResidualLoss,
//     fno/losses.py:367-467), forward and backward, on the time-last tensors (b, n, n, T) in place;
//   * one p-norm reduction (LpLoss, the main term of L2Loss2d, BochnerNorm) with its elementwise backward;
//   * the H^1 term of L2Loss2d: zero-padded central differences against a target gradient, with its backward.
//
// ---- the residual ---------------------------------------------------------------------------------------------------
// The reference runs eleven complex 3-D transforms over (n, n, T).  The time transforms cancel everywhere but in the
// 2 pi i kt term and in the final spectrum, so per time slice the work is 2-D, and one length-T DFT follows.  The multipliers
// 2 pi i kx, 2 pi i ky break Hermitian symmetry on the Nyquist row / column, so the four physical fields are COMPLEX: every
// transform here is complex to complex on full n x n planes (b, t, x, ky) of the workspace.  With F-(.) / F+(.) the
// unnormalised transforms of sign -1 / +1, m_k = 2 pi k, c_kt = 2 pi kt and lap the reference's patched table:
//
//   k_res_rows_fwd   Wr = F-_y(w)                                                     rows: one group of lanes per (b, x, t)
//   k_res_cols_mid   W = F-_x(Wr);  Psi = F+_x(-W / lap / n), Psix = F+_x(i m_kx . -W / lap / n), Wx = F+_x(i m_kx W / n),
//                    Lam = F+_x(visc lap W / n)                                        128-byte column tiles of one (b, t) plane
//   k_res_rows_mid   q = F+_y(i m_ky Psi / n), v = F+_y(-Psix / n), wx = F+_y(Wx / n), wy = F+_y(i m_ky Wr / n);
//                    U = F-_y(q wx + v wy - f) - Lam                                   (in place over Lam)
//   k_res_time       V_kt = sum_t e^{-2 pi i kt t / T} (U_t + i c_kt Wr_t)             dense DFT, T x 64 (32)-point chunks through LDS
//   k_res_cols_last  Re F-_x(V), squared, summed over the tile's ky per kx, in double  (no spectrum is written)
//   k_res_rowsum     S(b, kx) = the sums over (kt, tiles) in a fixed order
//   k_res_finish     out = scale * sum_{b, kx} sqrt(S)                                 (scale = fft-norm factor / (b n n))
//
// No floating-point atomics: the result is the same bit for bit from run to run.  The backward pass recomputes the planes
// (nothing but S is kept across the training step) and walks the same kernels' adjoints back:
//   k_res_cols_last_bwd  Vbar = F+_x(gout scale Re F-_x(V) / sqrt(S))      (0 where S = 0, as torch's norm)
//   k_res_time<adjoint>  Ubar_t = sum_kt conj(.) Vbar_kt,  Gw_t = sum_kt (-i c_kt) conj(.) Vbar_kt
//   k_res_rows_mid_bwd   pbar = F+_y(Ubar); grad f = -Re pbar; the four products with the conjugated partner fields, four F-_y:
//                        Psibar, Psixbar, Wxbar in place, Gw += (-i m_ky / n) F-_y(pbar conj v)
//   k_res_cols_mid_bwd   Gw += F+_x( conj(a0) F-_x Psibar + conj(a1) F-_x Psixbar + conj(a2) F-_x Wxbar - a3 F-_x Ubar )
//   k_res_rows_bwd       grad w = Re F+_y(Gw)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "tcfd_host.hpp"
#include "tcfd_fft.hpp"
#include "tcfd_loss_plan.hpp"

using namespace tcfd;

// elements per lane of the row transforms (one transform inside one wave) and of the column tiles: the loss kernels' choice
template <typename T, int N>
struct ResCfg {
    static constexpr int BASE = sizeof(T) == 8 ? 8 : 16;
    static constexpr int MIX = N % 3 == 0 ? 12 : (N % 5 == 0 ? 20 : 0);
    static constexpr int ROW_EPT0 = N >= 256 ? BASE : (N >= 64 ? 8 : 4);
    static constexpr int ROW_EPT = MIX ? MIX : (N / ROW_EPT0 > 64 ? N / 64 : ROW_EPT0);
    static constexpr int COLS = sizeof(T) == 8 ? 8 : 16;                    // 128-byte tile rows
    static constexpr int COL_EPT0 = N >= 256 ? BASE : (N >= 64 ? 8 : 4);
    static constexpr int COL_EPT = MIX ? MIX : (COLS * (N / COL_EPT0) > 1024 ? COLS * N / 1024 : COL_EPT0);
};

constexpr int ROW_THREADS = 256;    // threads of a row kernel's workgroup: ROW_THREADS / G transforms side by side
// (x, ky) points per workgroup of the time DFT: 2 * RES_MAX_NT * chunk complex numbers stay below 160 KB of LDS
template <typename T> constexpr int time_chunk() { return sizeof(T) == 8 ? 32 : 64; }
constexpr int RES_MAX_NT = 128;

// one group of G lanes per row (b, x, t); consecutive groups walk t first, so that a workgroup reads whole [y][t] lines of w / f
struct RowAddr {
    size_t slab;   // b * n + x
    int t;
    size_t row;    // first element of the plane row (b, t, x, :)
};
template <int Y>
__device__ __forceinline__ RowAddr row_addr(long gid, int nt) {
    RowAddr r;
    r.slab = (size_t)(gid / nt);
    r.t = (int)(gid - (long)r.slab * nt);
    const size_t b = r.slab / Y, x = r.slab - b * Y;
    r.row = ((b * nt + r.t) * Y + x) * Y;
    return r;
}

// ------------------------------------------------------------------ rows, forward: Wr = F-_y(w)
template <typename T, int Y, int EPT>
__global__ __launch_bounds__(ROW_THREADS) void k_res_rows_fwd(const T* __restrict__ w, cx<T>* __restrict__ Wr,
                                                              const cx<T>* __restrict__ tw, int nt, long ngroups) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int G = Y / EPT;
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const long gid = (long)blockIdx.x * (ROW_THREADS / G) + g;
    const bool live = gid < ngroups;
    const RowAddr a = row_addr<Y>(live ? gid : 0, nt);
    cf* lds = reinterpret_cast<cf*>(smem_raw) + (size_t)g * Y;
    const T* src = w + a.slab * Y * nt + a.t;
    cf z[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = mk<T>(src[(size_t)(j + e * G) * nt], (T)0);
    tile_fft<T, Y, EPT, -1, 1, true, 0>(z, lds, tw, j, 0);
    if (live) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) Wr[a.row + j + e * G] = z[e];
    }
}

// ------------------------------------------------------------------ columns, middle: the four multiplied fields back in (x, ky)
template <typename T, int X, int EPT, int C>
__global__ __launch_bounds__(C*(X / EPT)) void k_res_cols_mid(const cx<T>* __restrict__ Wr, cx<T>* __restrict__ Psi,
                                                              cx<T>* __restrict__ Psix, cx<T>* __restrict__ Wx,
                                                              cx<T>* __restrict__ Lam, const T* __restrict__ mkt,
                                                              const T* __restrict__ lap, const cx<T>* __restrict__ tw, T visc,
                                                              int ntiles) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* lds = reinterpret_cast<cf*>(smem_raw);
    constexpr int G = X / EPT;
    const int c = threadIdx.x % C, j = threadIdx.x / C;
    const int tile = blockIdx.x % ntiles;
    const size_t img = blockIdx.x / ntiles;                   // (b, t)
    const int q = tile * C + c;
    const T in = (T)1 / (T)X;
    cf W[EPT], z[EPT];
    T lp[EPT], mx[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        W[e] = Wr[(img * X + j + e * G) * X + q];
        lp[e] = lap[(size_t)(j + e * G) * X + q];
        mx[e] = mkt[j + e * G];
    }
    tile_fft<T, X, EPT, -1, C, false, 1>(W, lds, tw, j, c);
    // Psi
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = mk<T>(-(W[e].x / lp[e]) * in, -(W[e].y / lp[e]) * in);
    {
        cf zz[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) zz[e] = z[e];
        tile_fft<T, X, EPT, +1, C, false, 1>(zz, lds, tw, j, c);
#pragma unroll
        for (int e = 0; e < EPT; ++e) Psi[(img * X + j + e * G) * X + q] = zz[e];
    }
    // Psix = i m_kx psi^
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = cscale(mul_i(z[e]), mx[e]);
    tile_fft<T, X, EPT, +1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) Psix[(img * X + j + e * G) * X + q] = z[e];
    // Wx
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = cscale(mul_i(W[e]), mx[e] * in);
    tile_fft<T, X, EPT, +1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) Wx[(img * X + j + e * G) * X + q] = z[e];
    // Lam
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = cscale(W[e], visc * lp[e] * in);
    tile_fft<T, X, EPT, +1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) Lam[(img * X + j + e * G) * X + q] = z[e];
}

// ------------------------------------------------------------------ rows, middle: the product and its transform
template <typename T, int Y, int EPT>
__global__ __launch_bounds__(ROW_THREADS) void k_res_rows_mid(const cx<T>* __restrict__ Psi, const cx<T>* __restrict__ Psix,
                                                              const cx<T>* __restrict__ Wr, const cx<T>* __restrict__ Wx,
                                                              cx<T>* __restrict__ LU, const T* __restrict__ f,
                                                              const T* __restrict__ mkt, const cx<T>* __restrict__ tw, int nt,
                                                              long ngroups) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int G = Y / EPT;
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const long gid = (long)blockIdx.x * (ROW_THREADS / G) + g;
    const bool live = gid < ngroups;
    const RowAddr a = row_addr<Y>(live ? gid : 0, nt);
    cf* lds = reinterpret_cast<cf*>(smem_raw) + (size_t)g * Y;
    const T in = (T)1 / (T)Y;
    cf u[EPT], v[EPT], prod[EPT];
    // q = F+(i m_ky Psi / n), wx = F+(Wx / n)
#pragma unroll
    for (int e = 0; e < EPT; ++e) u[e] = cscale(mul_i(Psi[a.row + j + e * G]), mkt[j + e * G] * in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(u, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) v[e] = cscale(Wx[a.row + j + e * G], in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(v, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) prod[e] = cmul(u[e], v[e]);
    // v = F+(-Psix / n), wy = F+(i m_ky Wr / n)
#pragma unroll
    for (int e = 0; e < EPT; ++e) u[e] = cscale(Psix[a.row + j + e * G], -in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(u, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) v[e] = cscale(mul_i(Wr[a.row + j + e * G]), mkt[j + e * G] * in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(v, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) prod[e] = prod[e] + cmul(u[e], v[e]);
    if (f) {
        const T* fs = f + a.slab * Y * nt + a.t;
#pragma unroll
        for (int e = 0; e < EPT; ++e) prod[e].x -= fs[(size_t)(j + e * G) * nt];
    }
    tile_fft<T, Y, EPT, -1, 1, true, 0>(prod, lds, tw, j, 0);
    if (live) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) LU[a.row + j + e * G] = prod[e] - LU[a.row + j + e * G];
    }
}

// ------------------------------------------------------------------ the time DFT (and its adjoint), in place
// planes (b, t, pos), pos = (x, ky).  Forward: A = U -> V, B = Wr (read).  Adjoint: A = Vbar -> Ubar, B = Gw (written).
template <typename T, bool ADJ>
__global__ __launch_bounds__(256) void k_res_time(cx<T>* __restrict__ A, cx<T>* __restrict__ B, const cx<T>* __restrict__ twt,
                                                  const T* __restrict__ ckt, int nt, size_t plane) {
    typedef cx<T> cf;
    constexpr int TIME_CHUNK = time_chunk<T>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* sa = reinterpret_cast<cf*>(smem_raw);                  // [nt][TIME_CHUNK]
    cf* sb = sa + (size_t)nt * TIME_CHUNK;                     // forward only
    cf* stw = sa + (size_t)(ADJ ? 1 : 2) * nt * TIME_CHUNK;    // [nt]
    const size_t b = blockIdx.y, pos0 = (size_t)blockIdx.x * TIME_CHUNK;
    const int total = nt * TIME_CHUNK;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int t = i / TIME_CHUNK, p = i - t * TIME_CHUNK;
        const size_t o = (b * nt + t) * plane + pos0 + p;
        sa[i] = A[o];
        if (!ADJ) sb[i] = B[o];
    }
    for (int i = threadIdx.x; i < nt; i += 256) stw[i] = twt[i];
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += 256) {
        const int k = i / TIME_CHUNK, p = i - k * TIME_CHUNK;   // output index: kt (forward) or t (adjoint)
        const size_t o = (b * nt + k) * plane + pos0 + p;
        int idx = 0;
        if (!ADJ) {
            cf su = mk<T>((T)0, (T)0), sw = su;
            for (int t = 0; t < nt; ++t) {
                const cf wv = stw[idx];
                su = su + cmul(wv, sa[t * TIME_CHUNK + p]);
                sw = sw + cmul(wv, sb[t * TIME_CHUNK + p]);
                idx += k;
                if (idx >= nt) idx -= nt;
            }
            A[o] = su + cscale(mul_i(sw), ckt[k]);
        } else {
            cf su = mk<T>((T)0, (T)0), sw = su;
            for (int kt = 0; kt < nt; ++kt) {
                const cf wv = cconj(stw[idx]);
                const cf val = cmul(wv, sa[kt * TIME_CHUNK + p]);
                su = su + val;
                sw = sw + cscale(mul_mi(val), ckt[kt]);
                idx += k;
                if (idx >= nt) idx -= nt;
            }
            A[o] = su;
            B[o] = sw;
        }
    }
}

// ------------------------------------------------------------------ columns, last: Re F-_x(V), squared row sums of the tile
template <typename T, int X, int EPT, int C>
__global__ __launch_bounds__(C*(X / EPT)) void k_res_cols_last(const cx<T>* __restrict__ V, double* __restrict__ partial,
                                                               const cx<T>* __restrict__ tw, int ntiles) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* lds = reinterpret_cast<cf*>(smem_raw);
    constexpr int G = X / EPT;
    const int c = threadIdx.x % C, j = threadIdx.x / C;
    const int tile = blockIdx.x % ntiles;
    const size_t img = blockIdx.x / ntiles;                   // (b, kt)
    const int q = tile * C + c;
    cf z[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = V[(img * X + j + e * G) * X + q];
    tile_fft<T, X, EPT, -1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        double d = (double)z[e].x * (double)z[e].x;
#pragma unroll
        for (int off = C / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);     // the C columns of a row sit in adjacent lanes
        if (c == 0) partial[(img * ntiles + tile) * X + j + e * G] = d;
    }
}

// S(b, kx) = sum over (kt, tile) of the partial sums, in a fixed order
static __global__ __launch_bounds__(256) void k_res_rowsum(const double* __restrict__ partial, double* __restrict__ rows, long batch,
                                                    int n, int nt, int ntiles) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= batch * n) return;
    const long b = i / n, kx = i - b * n;
    double s = 0.0;
    const int terms = nt * ntiles;
    for (int k = 0; k < terms; ++k) s += partial[((size_t)b * terms + k) * n + kx];
    rows[i] = s;
}

template <typename T>
__global__ __launch_bounds__(256) void k_res_finish(const double* __restrict__ rows, T* __restrict__ out, long count, double scale) {
    __shared__ double red[256];
    double mine = 0.0;
    for (long i = threadIdx.x; i < count; i += 256) mine += sqrt(rows[i]);
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (T)(red[0] * scale);
}

// ------------------------------------------------------------------ backward kernels
template <typename T, int X, int EPT, int C>
__global__ __launch_bounds__(C*(X / EPT)) void k_res_cols_last_bwd(cx<T>* __restrict__ V, const double* __restrict__ rows,
                                                                   const T* __restrict__ gout, const cx<T>* __restrict__ tw,
                                                                   int ntiles, int nt, double scale) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* lds = reinterpret_cast<cf*>(smem_raw);
    constexpr int G = X / EPT;
    const int c = threadIdx.x % C, j = threadIdx.x / C;
    const int tile = blockIdx.x % ntiles;
    const size_t img = blockIdx.x / ntiles;                   // (b, kt)
    const size_t b = img / nt;
    const int q = tile * C + c;
    cf z[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = V[(img * X + j + e * G) * X + q];
    const double g = (double)gout[0] * scale;
    tile_fft<T, X, EPT, -1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const double s = rows[b * X + j + e * G];
        const double coef = s > 0.0 ? g / sqrt(s) : 0.0;      // a row of norm zero: zero gradient, as torch's norm
        z[e] = mk<T>((T)((double)z[e].x * coef), (T)0);
    }
    tile_fft<T, X, EPT, +1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) V[(img * X + j + e * G) * X + q] = z[e];
}

// Ubar in LU; Psi, Psix, Wx become their cotangents in place; Gw accumulates; grad f (optional)
template <typename T, int Y, int EPT>
__global__ __launch_bounds__(ROW_THREADS) void k_res_rows_mid_bwd(cx<T>* __restrict__ Psi, cx<T>* __restrict__ Psix,
                                                                  const cx<T>* __restrict__ Wr, cx<T>* __restrict__ Wx,
                                                                  const cx<T>* __restrict__ LU, cx<T>* __restrict__ Gw,
                                                                  T* __restrict__ gf, const T* __restrict__ mkt,
                                                                  const cx<T>* __restrict__ tw, int nt, long ngroups, int want_w) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int G = Y / EPT;
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const long gid = (long)blockIdx.x * (ROW_THREADS / G) + g;
    const bool live = gid < ngroups;
    const RowAddr a = row_addr<Y>(live ? gid : 0, nt);
    cf* lds = reinterpret_cast<cf*>(smem_raw) + (size_t)g * Y;
    const T in = (T)1 / (T)Y;
    cf pb[EPT], u[EPT], v[EPT], r[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) pb[e] = LU[a.row + j + e * G];
    tile_fft<T, Y, EPT, +1, 1, true, 0>(pb, lds, tw, j, 0);
    group_sync<0>();
    if (gf && live) {
        T* fs = gf + a.slab * Y * nt + a.t;
#pragma unroll
        for (int e = 0; e < EPT; ++e) fs[(size_t)(j + e * G) * nt] = -pb[e].x;
    }
    if (!want_w) return;
    // pair 1: q (from Psi) and wx (from Wx)
#pragma unroll
    for (int e = 0; e < EPT; ++e) u[e] = cscale(mul_i(Psi[a.row + j + e * G]), mkt[j + e * G] * in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(u, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) v[e] = cscale(Wx[a.row + j + e * G], in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(v, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = cmul(pb[e], cconj(v[e]));           // qbar
    tile_fft<T, Y, EPT, -1, 1, true, 0>(r, lds, tw, j, 0);
    group_sync<0>();
    if (live) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) Psi[a.row + j + e * G] = cscale(mul_mi(r[e]), mkt[j + e * G] * in);
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = cmul(pb[e], cconj(u[e]));           // wxbar
    tile_fft<T, Y, EPT, -1, 1, true, 0>(r, lds, tw, j, 0);
    group_sync<0>();
    if (live) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) Wx[a.row + j + e * G] = cscale(r[e], in);
    }
    // pair 2: v (from Psix) and wy (from Wr)
#pragma unroll
    for (int e = 0; e < EPT; ++e) u[e] = cscale(Psix[a.row + j + e * G], -in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(u, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) v[e] = cscale(mul_i(Wr[a.row + j + e * G]), mkt[j + e * G] * in);
    tile_fft<T, Y, EPT, +1, 1, true, 0>(v, lds, tw, j, 0);
    group_sync<0>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = cmul(pb[e], cconj(v[e]));           // vbar
    tile_fft<T, Y, EPT, -1, 1, true, 0>(r, lds, tw, j, 0);
    group_sync<0>();
    if (live) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) Psix[a.row + j + e * G] = cscale(r[e], -in);
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = cmul(pb[e], cconj(u[e]));           // wybar
    tile_fft<T, Y, EPT, -1, 1, true, 0>(r, lds, tw, j, 0);
    if (live) {
#pragma unroll
        for (int e = 0; e < EPT; ++e)
            Gw[a.row + j + e * G] = Gw[a.row + j + e * G] + cscale(mul_mi(r[e]), mkt[j + e * G] * in);
    }
}

template <typename T, int X, int EPT, int C>
__global__ __launch_bounds__(C*(X / EPT)) void k_res_cols_mid_bwd(const cx<T>* __restrict__ Psi, const cx<T>* __restrict__ Psix,
                                                                  const cx<T>* __restrict__ Wx, const cx<T>* __restrict__ LU,
                                                                  cx<T>* __restrict__ Gw, const T* __restrict__ mkt,
                                                                  const T* __restrict__ lap, const cx<T>* __restrict__ tw, T visc,
                                                                  int ntiles) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf* lds = reinterpret_cast<cf*>(smem_raw);
    constexpr int G = X / EPT;
    const int c = threadIdx.x % C, j = threadIdx.x / C;
    const int tile = blockIdx.x % ntiles;
    const size_t img = blockIdx.x / ntiles;                   // (b, t)
    const int q = tile * C + c;
    const T in = (T)1 / (T)X;
    cf acc[EPT], z[EPT];
    T lp[EPT], mx[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        lp[e] = lap[(size_t)(j + e * G) * X + q];
        mx[e] = mkt[j + e * G];
        z[e] = Psi[(img * X + j + e * G) * X + q];
    }
    tile_fft<T, X, EPT, -1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = mk<T>(-(z[e].x / lp[e]) * in, -(z[e].y / lp[e]) * in);            // a0 = -1 / (lap n)
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = Psix[(img * X + j + e * G) * X + q];
    tile_fft<T, X, EPT, -1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {                                                                          // conj(a1) = -i m a0
        const cf t = mul_mi(z[e]);
        acc[e] = acc[e] + mk<T>(-(t.x / lp[e]) * in * mx[e], -(t.y / lp[e]) * in * mx[e]);
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = Wx[(img * X + j + e * G) * X + q];
    tile_fft<T, X, EPT, -1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = acc[e] + cscale(mul_mi(z[e]), mx[e] * in);                        // conj(a2) = -i m / n
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = LU[(img * X + j + e * G) * X + q];
    tile_fft<T, X, EPT, -1, C, false, 1>(z, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) acc[e] = acc[e] - cscale(z[e], visc * lp[e] * in);                         // Lambar = -Ubar
    tile_fft<T, X, EPT, +1, C, false, 1>(acc, lds, tw, j, c);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const size_t o = (img * X + j + e * G) * X + q;
        Gw[o] = Gw[o] + acc[e];
    }
}

template <typename T, int Y, int EPT>
__global__ __launch_bounds__(ROW_THREADS) void k_res_rows_bwd(const cx<T>* __restrict__ Gw, T* __restrict__ gw,
                                                              const cx<T>* __restrict__ tw, int nt, long ngroups) {
    typedef cx<T> cf;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int G = Y / EPT;
    const int g = threadIdx.x / G, j = threadIdx.x % G;
    const long gid = (long)blockIdx.x * (ROW_THREADS / G) + g;
    const bool live = gid < ngroups;
    const RowAddr a = row_addr<Y>(live ? gid : 0, nt);
    cf* lds = reinterpret_cast<cf*>(smem_raw) + (size_t)g * Y;
    cf z[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) z[e] = Gw[a.row + j + e * G];
    tile_fft<T, Y, EPT, +1, 1, true, 0>(z, lds, tw, j, 0);
    if (live) {
        T* dst = gw + a.slab * Y * nt + a.t;
#pragma unroll
        for (int e = 0; e < EPT; ++e) dst[(size_t)(j + e * G) * nt] = z[e].x;
    }
}

// ------------------------------------------------------------------ host side of the residual
struct ResLayout {
    size_t plane_bytes;    // one complex plane set (b, t, n, n), 256-byte aligned
    size_t partial_off;    // doubles (b, t, ntiles, n)
    size_t total;
    int ntiles;
};
static ResLayout res_layout(const tcfd_loss_plan* p, long batch, int nt, int backward) {
    ResLayout L;
    const size_t cs = p->dtype == TCFD_C128 ? 16 : 8;
    const int C = p->dtype == TCFD_C128 ? 8 : 16;
    L.ntiles = p->n / C;
    L.plane_bytes = align256((size_t)batch * nt * p->n * p->n * cs);
    L.partial_off = (size_t)(backward ? 6 : 5) * L.plane_bytes;
    L.total = L.partial_off + align256((size_t)batch * nt * L.ntiles * p->n * sizeof(double));
    return L;
}

extern "C" size_t tcfd_residual_workspace_bytes(const tcfd_loss_plan* p, long batch, int nt, int backward) {
    if (!p || batch <= 0 || nt <= 0) return 0;
    return res_layout(p, batch, nt, backward).total;
}

extern "C" int tcfd_residual_loss_supported(const tcfd_loss_plan* p, int nt) {
    return (p && nt >= 1 && nt <= RES_MAX_NT) ? 1 : 0;
}

struct ResArgs {
    const void *w, *f, *m2pi, *lap, *ckt, *twt;
    double visc, scale;
    long batch;
    int nt;
};

// the launches both passes share: everything up to V (in plane 4); planes 0..3 = Wr, Psi, Psix, Wx
template <typename T, int N>
static int res_front(const tcfd_loss_plan* p, const ResArgs& a, void* ws, const ResLayout& L, hipStream_t st) {
    typedef cx<T> cf;
    constexpr int REPT = ResCfg<T, N>::ROW_EPT, CEPT = ResCfg<T, N>::COL_EPT, C = ResCfg<T, N>::COLS;
    constexpr int G = N / REPT, GPB = ROW_THREADS / G, TIME_CHUNK = time_chunk<T>();
    static_assert(G <= 64 && ROW_THREADS % G == 0, "a row transform lives in one wave");
    unsigned char* base = (unsigned char*)ws;
    cf* Wr = (cf*)base;
    cf* Psi = (cf*)(base + L.plane_bytes);
    cf* Psix = (cf*)(base + 2 * L.plane_bytes);
    cf* Wx = (cf*)(base + 3 * L.plane_bytes);
    cf* LU = (cf*)(base + 4 * L.plane_bytes);
    const cf* tw = (const cf*)p->tw;
    const long ngroups = a.batch * N * a.nt;
    const long rblocks = (ngroups + GPB - 1) / GPB;
    const long cblocks = a.batch * a.nt * L.ntiles;
    if (rblocks >= 2147483647L || cblocks >= 2147483647L || a.batch > 65535) return FAIL(TCFD_EINVAL, "residual_loss: too many blocks");
    const size_t lds_r = (size_t)GPB * N * sizeof(cf), lds_c = (size_t)N * C * sizeof(cf);
    int rc;
    {
        auto kern = k_res_rows_fwd<T, N, REPT>;
        if ((rc = raise_lds(kern, lds_r))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)rblocks), dim3(ROW_THREADS), lds_r, st, (const T*)a.w, Wr, tw, a.nt, ngroups);
        HIP_TRY(hipGetLastError());
    }
    {
        auto kern = k_res_cols_mid<T, N, CEPT, C>;
        if ((rc = raise_lds(kern, lds_c))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)cblocks), dim3(C * (N / CEPT)), lds_c, st, (const cf*)Wr, Psi, Psix, Wx, LU,
                           (const T*)a.m2pi, (const T*)a.lap, tw, (T)a.visc, L.ntiles);
        HIP_TRY(hipGetLastError());
    }
    {
        auto kern = k_res_rows_mid<T, N, REPT>;
        if ((rc = raise_lds(kern, lds_r))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)rblocks), dim3(ROW_THREADS), lds_r, st, (const cf*)Psi, (const cf*)Psix,
                           (const cf*)Wr, (const cf*)Wx, LU, (const T*)a.f, (const T*)a.m2pi, tw, a.nt, ngroups);
        HIP_TRY(hipGetLastError());
    }
    {
        auto kern = k_res_time<T, false>;
        const size_t lds_t = ((size_t)2 * a.nt * TIME_CHUNK + a.nt) * sizeof(cf);
        if ((rc = raise_lds(kern, lds_t))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)((size_t)N * N / TIME_CHUNK), (unsigned)a.batch), dim3(256), lds_t, st, LU, Wr,
                           (const cf*)a.twt, (const T*)a.ckt, a.nt, (size_t)N * N);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

template <typename T, int N>
static int res_fwd_impl(const tcfd_loss_plan* p, const ResArgs& a, void* out, void* rows, void* ws, hipStream_t st) {
    typedef cx<T> cf;
    constexpr int CEPT = ResCfg<T, N>::COL_EPT, C = ResCfg<T, N>::COLS;
    const ResLayout L = res_layout(p, a.batch, a.nt, 0);
    int rc = res_front<T, N>(p, a, ws, L, st);
    if (rc) return rc;
    unsigned char* base = (unsigned char*)ws;
    const cf* V = (const cf*)(base + 4 * L.plane_bytes);
    double* partial = (double*)(base + L.partial_off);
    {
        auto kern = k_res_cols_last<T, N, CEPT, C>;
        const size_t lds_c = (size_t)N * C * sizeof(cf);
        if ((rc = raise_lds(kern, lds_c))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)(a.batch * a.nt * L.ntiles)), dim3(C * (N / CEPT)), lds_c, st, V, partial,
                           (const cf*)p->tw, L.ntiles);
        HIP_TRY(hipGetLastError());
    }
    const long count = a.batch * N;
    hipLaunchKernelGGL(k_res_rowsum, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double*)partial, (double*)rows,
                       a.batch, N, a.nt, L.ntiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_res_finish<T>, dim3(1), dim3(256), 0, st, (const double*)rows, (T*)out, count, a.scale);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T, int N>
static int res_bwd_impl(const tcfd_loss_plan* p, const ResArgs& a, const void* rows, const void* gout, void* gw, void* gf, void* ws,
                        hipStream_t st) {
    typedef cx<T> cf;
    constexpr int REPT = ResCfg<T, N>::ROW_EPT, CEPT = ResCfg<T, N>::COL_EPT, C = ResCfg<T, N>::COLS;
    constexpr int G = N / REPT, GPB = ROW_THREADS / G, TIME_CHUNK = time_chunk<T>();
    const ResLayout L = res_layout(p, a.batch, a.nt, 1);
    int rc = res_front<T, N>(p, a, ws, L, st);
    if (rc) return rc;
    unsigned char* base = (unsigned char*)ws;
    cf* Wr = (cf*)base;
    cf* Psi = (cf*)(base + L.plane_bytes);
    cf* Psix = (cf*)(base + 2 * L.plane_bytes);
    cf* Wx = (cf*)(base + 3 * L.plane_bytes);
    cf* LU = (cf*)(base + 4 * L.plane_bytes);
    cf* Gw = (cf*)(base + 5 * L.plane_bytes);
    const cf* tw = (const cf*)p->tw;
    const long ngroups = a.batch * N * a.nt;
    const unsigned rblocks = (unsigned)((ngroups + GPB - 1) / GPB);
    const unsigned cblocks = (unsigned)(a.batch * a.nt * L.ntiles);
    const size_t lds_r = (size_t)GPB * N * sizeof(cf), lds_c = (size_t)N * C * sizeof(cf);
    {
        auto kern = k_res_cols_last_bwd<T, N, CEPT, C>;
        if ((rc = raise_lds(kern, lds_c))) return rc;
        hipLaunchKernelGGL(kern, dim3(cblocks), dim3(C * (N / CEPT)), lds_c, st, LU, (const double*)rows, (const T*)gout, tw,
                           L.ntiles, a.nt, a.scale);
        HIP_TRY(hipGetLastError());
    }
    {
        auto kern = k_res_time<T, true>;
        const size_t lds_t = ((size_t)a.nt * TIME_CHUNK + a.nt) * sizeof(cf);
        if ((rc = raise_lds(kern, lds_t))) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)((size_t)N * N / TIME_CHUNK), (unsigned)a.batch), dim3(256), lds_t, st, LU, Gw,
                           (const cf*)a.twt, (const T*)a.ckt, a.nt, (size_t)N * N);
        HIP_TRY(hipGetLastError());
    }
    {
        auto kern = k_res_rows_mid_bwd<T, N, REPT>;
        if ((rc = raise_lds(kern, lds_r))) return rc;
        hipLaunchKernelGGL(kern, dim3(rblocks), dim3(ROW_THREADS), lds_r, st, Psi, Psix, (const cf*)Wr, Wx, (const cf*)LU, Gw,
                           (T*)gf, (const T*)a.m2pi, tw, a.nt, ngroups, gw ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    if (!gw) return 0;
    {
        auto kern = k_res_cols_mid_bwd<T, N, CEPT, C>;
        if ((rc = raise_lds(kern, lds_c))) return rc;
        hipLaunchKernelGGL(kern, dim3(cblocks), dim3(C * (N / CEPT)), lds_c, st, (const cf*)Psi, (const cf*)Psix, (const cf*)Wx,
                           (const cf*)LU, Gw, (const T*)a.m2pi, (const T*)a.lap, tw, (T)a.visc, L.ntiles);
        HIP_TRY(hipGetLastError());
    }
    {
        auto kern = k_res_rows_bwd<T, N, REPT>;
        if ((rc = raise_lds(kern, lds_r))) return rc;
        hipLaunchKernelGGL(kern, dim3(rblocks), dim3(ROW_THREADS), lds_r, st, (const cf*)Gw, (T*)gw, tw, a.nt, ngroups);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

#define TCFD_RES_SIZES(M)                                                                                                   \
    M(16) M(32) M(64) M(128) M(256) M(512) M(1024) M(96) M(192) M(384) M(768) M(80) M(160) M(320) M(640)

template <typename T>
static int res_fwd_dispatch(const tcfd_loss_plan* p, const ResArgs& a, void* out, void* rows, void* ws, hipStream_t st) {
#define TCFD_RES_CASE(N_) case N_: return res_fwd_impl<T, N_>(p, a, out, rows, ws, st);
    switch (p->n) { TCFD_RES_SIZES(TCFD_RES_CASE) }
#undef TCFD_RES_CASE
    return FAIL(TCFD_EINVAL, "residual_loss: unsupported n = %d", p->n);
}
template <typename T>
static int res_bwd_dispatch(const tcfd_loss_plan* p, const ResArgs& a, const void* rows, const void* gout, void* gw, void* gf,
                            void* ws, hipStream_t st) {
#define TCFD_RES_CASE(N_) case N_: return res_bwd_impl<T, N_>(p, a, rows, gout, gw, gf, ws, st);
    switch (p->n) { TCFD_RES_SIZES(TCFD_RES_CASE) }
#undef TCFD_RES_CASE
    return FAIL(TCFD_EINVAL, "residual_loss_backward: unsupported n = %d", p->n);
}

extern "C" int tcfd_residual_loss(const tcfd_loss_plan* p, const void* w, const void* f, const void* mk2pi, const void* lap,
                                  const void* ckt, const void* twt, double visc, double scale, long batch, int nt, void* out,
                                  void* rows, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || !mk2pi || !lap || !ckt || !twt || !out || !rows || !ws) return FAIL(TCFD_EINVAL, "residual_loss: null argument");
    if (batch <= 0 || !tcfd_residual_loss_supported(p, nt)) return FAIL(TCFD_EINVAL, "residual_loss: bad sizes (batch %ld, nt %d)", batch, nt);
    const size_t need = tcfd_residual_workspace_bytes(p, batch, nt, 0);
    if (ws_bytes < need) return FAIL(TCFD_EWORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
    const ResArgs a{w, f, mk2pi, lap, ckt, twt, visc, scale, batch, nt};
    if (p->dtype == TCFD_C128) return res_fwd_dispatch<double>(p, a, out, rows, ws, (hipStream_t)stream);
    return res_fwd_dispatch<float>(p, a, out, rows, ws, (hipStream_t)stream);
}

extern "C" int tcfd_residual_loss_backward(const tcfd_loss_plan* p, const void* w, const void* f, const void* mk2pi,
                                           const void* lap, const void* ckt, const void* twt, double visc, double scale,
                                           const void* rows, const void* gout, long batch, int nt, void* grad_w, void* grad_f,
                                           void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || !mk2pi || !lap || !ckt || !twt || !rows || !gout || !ws || (!grad_w && !grad_f))
        return FAIL(TCFD_EINVAL, "residual_loss_backward: null argument");
    if (batch <= 0 || !tcfd_residual_loss_supported(p, nt))
        return FAIL(TCFD_EINVAL, "residual_loss_backward: bad sizes (batch %ld, nt %d)", batch, nt);
    const size_t need = tcfd_residual_workspace_bytes(p, batch, nt, 1);
    if (ws_bytes < need) return FAIL(TCFD_EWORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
    const ResArgs a{w, f, mk2pi, lap, ckt, twt, visc, scale, batch, nt};
    if (p->dtype == TCFD_C128) return res_bwd_dispatch<double>(p, a, rows, gout, grad_w, grad_f, ws, (hipStream_t)stream);
    return res_bwd_dispatch<float>(p, a, rows, gout, grad_w, grad_f, ws, (hipStream_t)stream);
}

// ===================================================================== p-norm sums
// x, y viewed as (outer, reduce, inner), contiguous.  sd[o][i] = sum_r |x - y|^p (y may be null: |x|^p), sy[o][i] = sum_r |y|^p
// (when asked).  Stage 1: `nblk` workgroups per outer index walk equal contiguous shares; a lane keeps its `inner` index (the
// stride TB is a multiple of inner).  Stage 2 adds the nblk partial sums in a fixed order.  Double accumulators throughout.
__device__ __forceinline__ double lp_pow(double a, double p, int mode) {
    a = fabs(a);
    return mode == 1 ? a : (mode == 2 ? a * a : pow(a, p));
}

template <typename T>
__global__ __launch_bounds__(256) void k_lp_partial(const T* __restrict__ x, const T* __restrict__ y, double* __restrict__ part,
                                                    long reduce, int inner, int nblk, double p, int mode, int want_y) {
    __shared__ double rd[256], ry[256];
    const int TB = (256 / inner) * inner;
    const long o = blockIdx.y;
    const long per = (reduce + nblk - 1) / nblk;
    const long r0 = (long)blockIdx.x * per, r1 = r0 + per < reduce ? r0 + per : reduce;
    const size_t base = (size_t)o * reduce * inner;
    double ad = 0.0, ay = 0.0;
    if ((int)threadIdx.x < TB) {
        for (long e = r0 * inner + threadIdx.x; e < r1 * inner; e += TB) {
            const double xv = (double)x[base + e];
            const double yv = y ? (double)y[base + e] : 0.0;
            ad += lp_pow(xv - yv, p, mode);
            if (want_y) ay += lp_pow(yv, p, mode);
        }
    }
    rd[threadIdx.x] = ad;
    ry[threadIdx.x] = ay;
    __syncthreads();
    if ((int)threadIdx.x < inner) {
        double sd = 0.0, sy = 0.0;
        for (int k = threadIdx.x; k < TB; k += inner) {
            sd += rd[k];
            sy += ry[k];
        }
        const size_t slot = (((size_t)o * nblk + blockIdx.x) * 2) * inner + threadIdx.x;
        part[slot] = sd;
        part[slot + inner] = sy;
    }
}

__global__ __launch_bounds__(256) void k_lp_final(const double* __restrict__ part, double* __restrict__ sd, double* __restrict__ sy,
                                                  long outer, int inner, int nblk) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= outer * inner) return;
    const long o = i / inner;
    const int c = (int)(i - o * inner);
    double a = 0.0, b = 0.0;
    for (int k = 0; k < nblk; ++k) {
        const size_t slot = (((size_t)o * nblk + k) * 2) * inner + c;
        a += part[slot];
        b += part[slot + inner];
    }
    sd[i] = a;
    if (sy) sy[i] = b;
}

// gx = cd[o][i] d/dx |x - y|^p;   gy = -that + cy[o][i] d/dy |y|^p   (cd, cy: doubles, the cotangents of the sums)
template <typename T>
__global__ __launch_bounds__(256) void k_lp_bwd(const T* __restrict__ x, const T* __restrict__ y, const double* __restrict__ cd,
                                                const double* __restrict__ cy, T* __restrict__ gx, T* __restrict__ gy,
                                                size_t per_outer, int inner, double p, int mode) {
    // blockIdx.y = the outer index: no 64-bit division per element
    const size_t o = blockIdx.y, base = o * per_outer;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < per_outer; r += (size_t)gridDim.x * 256) {
        const size_t e = base + r;
        const size_t slot = o * inner + (inner == 1 ? 0 : r % inner);
        const double xv = (double)x[e], yv = y ? (double)y[e] : 0.0;
        const double d = xv - yv;
        auto dpow = [&](double v) {
            if (v == 0.0) return 0.0;
            const double s = v > 0.0 ? 1.0 : -1.0;
            return mode == 1 ? s : (mode == 2 ? 2.0 * v : s * p * pow(fabs(v), p - 1.0));
        };
        // a zero derivative stays zero whatever the cotangent (inf at a vanishing norm): the subgradient torch's norm takes
        const double dd = dpow(d), dy = cy ? dpow(yv) : 0.0;
        const double g = dd == 0.0 ? 0.0 : cd[slot] * dd;
        if (gx) gx[e] = (T)g;
        if (gy) gy[e] = (T)(-g + (dy == 0.0 ? 0.0 : cy[slot] * dy));
    }
}

static int lp_nblk(long reduce, int inner) {
    const long elems = reduce * inner;
    long nb = (elems + 16383) / 16384;
    if (nb > 256) nb = 256;
    if (nb > reduce) nb = reduce;
    return (int)(nb < 1 ? 1 : nb);
}

extern "C" size_t tcfd_lp_sums_workspace_bytes(long outer, long reduce, int inner) {
    if (outer <= 0 || reduce <= 0 || inner <= 0) return 0;
    return align256((size_t)outer * lp_nblk(reduce, inner) * 2 * inner * sizeof(double));
}

extern "C" int tcfd_lp_sums(const void* x, const void* y, void* sum_diff, void* sum_y, long outer, long reduce, int inner, double p,
                            int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !sum_diff || !ws || (sum_y && !y)) return FAIL(TCFD_EINVAL, "lp_sums: null argument");
    if (outer <= 0 || outer > 65535 || reduce <= 0 || inner <= 0 || inner > 256 || !(p > 0.0) || !std::isfinite(p))
        return FAIL(TCFD_EINVAL, "lp_sums: bad sizes (outer %ld, reduce %ld, inner %d) or p = %g", outer, reduce, inner, p);
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return FAIL(TCFD_EINVAL, "lp_sums: bad dtype %d", dtype);
    const size_t need = tcfd_lp_sums_workspace_bytes(outer, reduce, inner);
    if (ws_bytes < need) return FAIL(TCFD_EWORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
    const int nblk = lp_nblk(reduce, inner);
    const int mode = p == 1.0 ? 1 : (p == 2.0 ? 2 : 0);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TCFD_C128)
        hipLaunchKernelGGL(k_lp_partial<double>, dim3(nblk, (unsigned)outer), dim3(256), 0, st, (const double*)x, (const double*)y,
                           (double*)ws, reduce, inner, nblk, p, mode, sum_y ? 1 : 0);
    else
        hipLaunchKernelGGL(k_lp_partial<float>, dim3(nblk, (unsigned)outer), dim3(256), 0, st, (const float*)x, (const float*)y,
                           (double*)ws, reduce, inner, nblk, p, mode, sum_y ? 1 : 0);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lp_final, dim3((unsigned)((outer * inner + 255) / 256)), dim3(256), 0, st, (const double*)ws,
                       (double*)sum_diff, (double*)sum_y, outer, inner, nblk);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int tcfd_lp_sums_bwd(const void* x, const void* y, const void* cot_diff, const void* cot_y, void* grad_x, void* grad_y,
                                long outer, long reduce, int inner, double p, int dtype, void* stream) {
    if (!x || !cot_diff || (!grad_x && !grad_y) || (grad_y && !y)) return FAIL(TCFD_EINVAL, "lp_sums_bwd: null argument");
    if (outer <= 0 || reduce <= 0 || inner <= 0 || !(p > 0.0) || !std::isfinite(p)) return FAIL(TCFD_EINVAL, "lp_sums_bwd: bad sizes");
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return FAIL(TCFD_EINVAL, "lp_sums_bwd: bad dtype %d", dtype);
    if (outer > 65535) return FAIL(TCFD_EINVAL, "lp_sums_bwd: outer %ld > 65535", outer);
    const size_t per_outer = (size_t)reduce * inner;
    const int mode = p == 1.0 ? 1 : (p == 2.0 ? 2 : 0);
    const dim3 blocks((unsigned)std::min<size_t>((per_outer + 255) / 256, 4096), (unsigned)outer);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TCFD_C128)
        hipLaunchKernelGGL(k_lp_bwd<double>, blocks, dim3(256), 0, st, (const double*)x, (const double*)y, (const double*)cot_diff,
                           (const double*)cot_y, (double*)grad_x, (double*)grad_y, per_outer, inner, p, mode);
    else
        hipLaunchKernelGGL(k_lp_bwd<float>, blocks, dim3(256), 0, st, (const float*)x, (const float*)y, (const double*)cot_diff,
                           (const double*)cot_y, (float*)grad_x, (float*)grad_y, per_outer, inner, p, mode);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ===================================================================== the H^1 term of L2Loss2d
// preds (N, C, n1, n2), tgrad (N, 2 C, n1, n2): channels [0, C) = d/d(dim -2), [C, 2 C) = d/d(dim -1).  ksqrt: null, or the
// square root of the diffusion constant, one value (kmode 1) or (N, 1, n1, n2) (kmode 2).
//   s1[N] = sum (ksqrt (cd(preds) - tgrad))^2,   s2[N] = sum ksqrt tgrad^2        cd = zero-padded central difference / h
template <typename T>
__device__ __forceinline__ T h1_at(const T* __restrict__ p, int i, int j, int n1, int n2) {
    return (i >= 0 && i < n1 && j >= 0 && j < n2) ? p[(size_t)i * n2 + j] : (T)0;
}
template <typename T>
__device__ __forceinline__ T h1_k(const T* __restrict__ ks, int kmode, size_t n, size_t ij, size_t img) {
    return kmode == 0 ? (T)1 : (kmode == 1 ? ks[0] : ks[n * img + ij]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_h1_partial(const T* __restrict__ preds, const T* __restrict__ tgrad,
                                                    const T* __restrict__ ks, double* __restrict__ part, int C, int n1, int n2,
                                                    T h, int kmode, int nblk) {
    __shared__ double r1[256], r2[256];
    const size_t n = blockIdx.y, img = (size_t)n1 * n2, per = (size_t)C * img;
    double a1 = 0.0, a2 = 0.0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)nblk * 256) {
        const size_t c = e / img, ij = e - c * img;
        const int i = (int)(ij / n2), j = (int)(ij - (size_t)i * n2);
        const T* p = preds + (n * C + c) * img;
        const T gx = ((h1_at(p, i + 1, j, n1, n2) - h1_at(p, i - 1, j, n1, n2)) / (T)2) / h;
        const T gy = ((h1_at(p, i, j + 1, n1, n2) - h1_at(p, i, j - 1, n1, n2)) / (T)2) / h;
        const T tx = tgrad[(n * 2 * C + c) * img + ij], ty = tgrad[(n * 2 * C + C + c) * img + ij];
        const T kk = h1_k(ks, kmode, n, ij, img);
        const double dx = (double)(kk * (gx - tx)), dy = (double)(kk * (gy - ty));
        a1 += dx * dx + dy * dy;
        a2 += (double)kk * ((double)tx * (double)tx + (double)ty * (double)ty);
    }
    r1[threadIdx.x] = a1;
    r2[threadIdx.x] = a2;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            r1[threadIdx.x] += r1[threadIdx.x + off];
            r2[threadIdx.x] += r2[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[(n * nblk + blockIdx.x) * 2] = r1[0];
        part[(n * nblk + blockIdx.x) * 2 + 1] = r2[0];
    }
}

// grad preds = cot[n] * d s1 / d preds: the adjoint stencil of r = 2 ksqrt^2 (cd(preds) - tgrad)
template <typename T>
__global__ __launch_bounds__(256) void k_h1_bwd(const T* __restrict__ preds, const T* __restrict__ tgrad, const T* __restrict__ ks,
                                                const double* __restrict__ cot, T* __restrict__ grad, int C, int n1, int n2, T h,
                                                int kmode, size_t total) {
    const size_t img = (size_t)n1 * n2;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t nc = e / img, ij = e - nc * img;
        const size_t n = nc / C, c = nc - n * C;
        const int i = (int)(ij / n2), j = (int)(ij - (size_t)i * n2);
        const T* p = preds + nc * img;
        const T* tx = tgrad + (n * 2 * C + c) * img;
        const T* ty = tgrad + (n * 2 * C + C + c) * img;
        auto rx = [&](int a, int b) -> double {      // r of the x-difference at (a, b); 0 outside
            if (a < 0 || a >= n1) return 0.0;
            const T g = ((h1_at(p, a + 1, b, n1, n2) - h1_at(p, a - 1, b, n1, n2)) / (T)2) / h;
            const T kk = h1_k(ks, kmode, n, (size_t)a * n2 + b, img);
            return 2.0 * (double)kk * (double)(kk * (g - tx[(size_t)a * n2 + b]));
        };
        auto ry = [&](int a, int b) -> double {
            if (b < 0 || b >= n2) return 0.0;
            const T g = ((h1_at(p, a, b + 1, n1, n2) - h1_at(p, a, b - 1, n1, n2)) / (T)2) / h;
            const T kk = h1_k(ks, kmode, n, (size_t)a * n2 + b, img);
            return 2.0 * (double)kk * (double)(kk * (g - ty[(size_t)a * n2 + b]));
        };
        const double v = (rx(i - 1, j) - rx(i + 1, j) + ry(i, j - 1) - ry(i, j + 1)) / (2.0 * (double)h);
        grad[e] = (T)(cot[n] * v);
    }
}

static int h1_nblk(long per) {
    long nb = (per + 8191) / 8192;
    return (int)(nb > 128 ? 128 : (nb < 1 ? 1 : nb));
}

extern "C" size_t tcfd_h1_sums_workspace_bytes(long batch, int channels, int n1, int n2) {
    if (batch <= 0 || channels <= 0 || n1 <= 0 || n2 <= 0) return 0;
    return align256((size_t)batch * h1_nblk((long)channels * n1 * n2) * 2 * sizeof(double));
}

extern "C" int tcfd_h1_sums(const void* preds, const void* tgrad, const void* ksqrt, int kmode, void* s1, void* s2, long batch,
                            int channels, int n1, int n2, double h, int dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!preds || !tgrad || !s1 || !s2 || !ws || (kmode != 0 && !ksqrt)) return FAIL(TCFD_EINVAL, "h1_sums: null argument");
    if (batch <= 0 || batch > 65535 || channels <= 0 || n1 <= 0 || n2 <= 0 || kmode < 0 || kmode > 2)
        return FAIL(TCFD_EINVAL, "h1_sums: bad sizes");
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return FAIL(TCFD_EINVAL, "h1_sums: bad dtype %d", dtype);
    const size_t need = tcfd_h1_sums_workspace_bytes(batch, channels, n1, n2);
    if (ws_bytes < need) return FAIL(TCFD_EWORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
    const int nblk = h1_nblk((long)channels * n1 * n2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TCFD_C128)
        hipLaunchKernelGGL(k_h1_partial<double>, dim3(nblk, (unsigned)batch), dim3(256), 0, st, (const double*)preds,
                           (const double*)tgrad, (const double*)ksqrt, (double*)ws, channels, n1, n2, h, kmode, nblk);
    else
        hipLaunchKernelGGL(k_h1_partial<float>, dim3(nblk, (unsigned)batch), dim3(256), 0, st, (const float*)preds,
                           (const float*)tgrad, (const float*)ksqrt, (double*)ws, channels, n1, n2, (float)h, kmode, nblk);
    HIP_TRY(hipGetLastError());
    // the (batch, nblk, 2) partial sums as an lp-style second stage: inner = 2 keeps s1 / s2 apart
    hipLaunchKernelGGL(k_lp_final, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, (const double*)ws, (double*)s1,
                       (double*)s2, batch, 1, nblk);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int tcfd_h1_sums_bwd(const void* preds, const void* tgrad, const void* ksqrt, int kmode, const void* cot, void* grad,
                                long batch, int channels, int n1, int n2, double h, int dtype, void* stream) {
    if (!preds || !tgrad || !cot || !grad || (kmode != 0 && !ksqrt)) return FAIL(TCFD_EINVAL, "h1_sums_bwd: null argument");
    if (batch <= 0 || channels <= 0 || n1 <= 0 || n2 <= 0 || kmode < 0 || kmode > 2) return FAIL(TCFD_EINVAL, "h1_sums_bwd: bad sizes");
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return FAIL(TCFD_EINVAL, "h1_sums_bwd: bad dtype %d", dtype);
    const size_t total = (size_t)batch * channels * n1 * n2;
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TCFD_C128)
        hipLaunchKernelGGL(k_h1_bwd<double>, dim3(blocks), dim3(256), 0, st, (const double*)preds, (const double*)tgrad,
                           (const double*)ksqrt, (const double*)cot, (double*)grad, channels, n1, n2, h, kmode, total);
    else
        hipLaunchKernelGGL(k_h1_bwd<float>, dim3(blocks), dim3(256), 0, st, (const float*)preds, (const float*)tgrad,
                           (const float*)ksqrt, (const double*)cot, (float*)grad, channels, n1, n2, (float)h, kmode, total);
    HIP_TRY(hipGetLastError());
    return 0;
}
