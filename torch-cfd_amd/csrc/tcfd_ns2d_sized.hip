// tcfd_ns2d_sized.hip -- MI355X (gfx950) kernels of the batched 2-D pseudo-spectral RK4-CN vorticity step: everything that is
// templated on the grid size, with its launchers and drivers.  See DESIGN.md for the pass model.  Built from scratch; the
// reference path (torch_cfd/equations.py:328-358, 413-463; torch_cfd/spectral.py:41-115) is a stream of ~200 ATen launches
// per step, here it is three kernels per RK stage:
//
//   k_cols  MODE_A  : u -> {u^,v^,dx w^,dy w^} -> column inverse FFT -> 4 planes
//   k_rows_advect   : 4 row c2r -> -(dx w * vx + dy w * vy) -> row r2c
//   k_cols  MODE_CA : column FFT -> mask, forcing, h <- F + beta h,
//                     u <- (u + g h + mu L u)/(1 - mu L) -> (MODE_A of next stage)
//
// Compiled TWICE, in parallel (torch-cfd_amd/_lib.py), with -DTCFD_REAL=double and -DTCFD_REAL=float: each object holds one
// precision's instantiations behind the ns2d:: templates of tcfd_ns2d_plan.hpp that the C ABI in tcfd_ns2d.hip calls (one unit
// with both took 7 minutes of hipcc).  Linked twice, so everything here is a template or has internal linkage; a kernel's launch
// and its hipFuncSetAttribute (set_lds, the function-local DevOnce objects) stay in the unit that instantiates it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "tcfd_ns2d_plan.hpp"

#ifndef TCFD_REAL
#error "build with -DTCFD_REAL=double or -DTCFD_REAL=float"
#endif

using namespace tcfd;

// ------------------------------------------------------------------ per-size configuration
// COL_EPT / ROW_EPT = elements per lane of one transform in the column / row kernels,
// COLS = columns per tile of the column kernels, ROW_THREADS = workgroup size of the row kernels.
// TCFD_NT_COL_IN=1 (build time): the advection a column pass transforms is read exactly once and dead afterwards
#ifndef TCFD_NT_COL_IN
#define TCFD_NT_COL_IN 0
#endif
#if TCFD_NT_COL_IN
#define TCFD_COL_LD(p_) load_stream(p_)
#else
#define TCFD_COL_LD(p_) (*(p_))
#endif
template <typename T, int N> struct Cfg;
#define TCFD_CFG(T, N, CEPT_, COLS_, REPT_, RTHR_)                                     \
    template <> struct Cfg<T, N> {                                                     \
        static constexpr int COL_EPT = CEPT_, COLS = COLS_, ROW_EPT = REPT_, ROW_THREADS = RTHR_; \
    };
TCFD_CFG(double, 8, 8, 64, 8, 256)
TCFD_CFG(double, 16, 4, 16, 4, 256)
TCFD_CFG(double, 32, 8, 32, 8, 256)
TCFD_CFG(double, 64, 8, 32, 8, 256)
TCFD_CFG(double, 128, 8, 16, 8, 256)
TCFD_CFG(double, 256, 16, 16, 16, 256)
TCFD_CFG(double, 512, 8, 8, 8, 256)
TCFD_CFG(double, 1024, 16, 8, 8, 128)
TCFD_CFG(double, 2048, 16, 2, 16, 256)
TCFD_CFG(float, 8, 8, 64, 8, 256)
TCFD_CFG(float, 16, 4, 16, 4, 256)
TCFD_CFG(float, 32, 8, 32, 8, 256)
TCFD_CFG(float, 64, 8, 32, 8, 256)
TCFD_CFG(float, 128, 8, 16, 8, 256)
TCFD_CFG(float, 256, 16, 16, 16, 256)
TCFD_CFG(float, 512, 8, 16, 8, 256)
TCFD_CFG(float, 1024, 16, 8, 16, 256)
TCFD_CFG(float, 2048, 16, 8, 16, 256)
// n = 4096: the step runs split (2048-point half columns in the tile forms of the two rows above); these whole-column tiles
// serve the passes that are never split (plain transforms, the VJP / JVP sweeps) and TCFD_SPLIT=0.  One (two) columns: the
// fp64 tile is 64 KB + 96 KB of row tables = the CU's whole LDS, the fp32 one 112 KB (four columns would be 176 KB)
TCFD_CFG(double, 4096, 16, 1, 16, 256)
TCFD_CFG(float, 4096, 16, 2, 16, 256)
// n = 3 * 2^k: twelve elements per lane (radix 12 = 4 x 3 in registers, then radix-4 passes), plain Stockham tiles
TCFD_CFG(double, 96, 12, 32, 12, 256)
TCFD_CFG(double, 192, 12, 16, 12, 256)
TCFD_CFG(double, 384, 12, 8, 12, 256)
TCFD_CFG(double, 768, 12, 8, 12, 256)
TCFD_CFG(float, 96, 12, 32, 12, 256)
TCFD_CFG(float, 192, 12, 16, 12, 256)
TCFD_CFG(float, 384, 12, 16, 12, 256)
TCFD_CFG(float, 768, 12, 16, 12, 256)
TCFD_CFG(double, 1536, 12, 4, 12, 256)     // 4 (8) columns: a whole-column tile of 8 (16) would not fit the LDS
TCFD_CFG(float, 1536, 12, 8, 12, 256)
// n = 5 * 2^k: twenty elements per lane (radix 20 = 4 x 5 in registers, then radix 4 / 2)
TCFD_CFG(double, 80, 20, 32, 20, 256)
TCFD_CFG(double, 160, 20, 16, 20, 256)
TCFD_CFG(double, 320, 20, 8, 20, 256)
TCFD_CFG(double, 640, 20, 8, 20, 256)
TCFD_CFG(float, 80, 20, 32, 20, 256)
TCFD_CFG(float, 160, 20, 16, 20, 256)
TCFD_CFG(float, 320, 20, 16, 20, 256)
TCFD_CFG(float, 640, 20, 16, 20, 256)
TCFD_CFG(double, 1280, 20, 4, 20, 256)
TCFD_CFG(float, 1280, 20, 8, 20, 256)

// ------------------------------------------------------------------ column kernels
enum ColMode {
    MODE_A = 0,     // u_in -> 4 planes
    MODE_CA = 1,    // adv -> FFT -> RK update (h, u_out) -> 4 planes
    MODE_C = 2,     // adv -> FFT -> RK update (h, u_out)
    MODE_F = 3,     // adv -> FFT -> out = mask*x + forcing
    MODE_RES = 4,   // adv -> FFT -> residual = wt - F - L w ; psi = -w/lap
    MODE_FWD = 5,   // generic column forward c2c:  in -> out * scale
    MODE_INV = 6    // generic column inverse c2c:  in -> out * scale
};

template <typename T>
struct ColArgs {
    const cx<T>* in;      // adv (MODE_CA/C/F/RES) or generic input
    const cx<T>* u_in;    // state read  (w for MODE_RES)
    const cx<T>* wt;      // MODE_RES only
    cx<T>* u_out;         // state write
    cx<T>* h;             // RK accumulator (read unless load_h == 0, written)
    cx<T>* planes;        // 4 output planes (MODE_A/CA)
    cx<T>* out;           // MODE_F / FWD / INV output ; MODE_RES residual
    cx<T>* psi;           // MODE_RES
    const cx<T>* w0;      // MODE_C with dwdt: the call's input (caller layout), dwdt = (u_new - w0) * dwdt_scale
    cx<T>* dwdt;          // or null
    const T* kx;          // [n]
    const T* ky;          // [m]
    const T* lin;         // [n*m]
    const T* mask;        // [n*m]
    const cx<T>* forcing; // [n*m] or null (dense form)
    // separable / sparse forms of the same tables (chosen at plan creation when they are exact):
    const T* mask_r;      // [n], mask = mask_r[i] * mask_c[j]
    const T* mask_c;      // [m]
    const T* lin_r;       // [n], linear_term = lin_r[i] + lin_c[j]
    const T* lin_c;       // [m]
    const int* f_ptr;     // [m+1] CSC column pointers of the non-zero forcing entries, or null
    const int* f_row;     // [nnz]
    const int* f_col;     // [nnz]
    const cx<T>* f_val;   // [nnz]
    int f_nnz;            // > 0: so few entries that every lane scans the whole list (uniform scalar loads)
    int sep;              // 1: use the separable mask / linear term
    int keep_cols;        // > 0: columns >= keep_cols and rows with mask_r == 0 carry F = h = 0 (pruned)
    const cx<T>* tw;      // [n]
    size_t plane_stride;  // elements between planes
    T beta, gdt, mu, scale;
    T dwdt_scale;
    T fa, mud;   // h <- fa F + beta h ;  u <- (base + gdt h + mu L base) / (1 - mud L)   (RK4-CN: fa = 1, mud = mu)
    int m;        // row pitch (elements) of caller-layout arrays: u_in, u_out, wt, out, psi
    int ldw;      // row pitch of workspace arrays (adv, h, planes): m rounded up to a 128-byte multiple
    int in_ld;    // MODE_FWD / MODE_INV: pitch of `in`
    int out_ld;   // MODE_FWD / MODE_INV: pitch of `out`
    int u_in_ld;  // MODE_A / CA / C: pitch of u_in (m for the caller's array, ldw for the internal state copy)
    int u_out_ld; // MODE_CA / C: pitch of u_out
    int ntiles;
    int batch;
    int load_h;
    int store_h;   // 0 at the last stage of a step: the accumulator is dead (the next step starts from h = 0)
    int ablate;    // timing ablations (TCFD_ABLATE bit mask; results are WRONG when non-zero): 1 skip the
                   // transforms, 2 skip the plane stores, 4 skip the table reads, 8 skip the h traffic,
                   // 64 skip the packing of the Nyquist column into the planes, 128 skip that column's update
    int nyq;       // 1: packed Nyquist column (see emit_planes): no lone tile for column m - 1, the lanes of column 0 own it too
    int nt_planes; // plane stores with the non-temporal hint (small cache-resident problems, see launch_cols)
    int nt_out;    // MODE_C: the new state and dw/dt go to the CALLER's arrays and are not read again by this call -- stored with
                   // the non-temporal hint they do not push the next chunk's working set out of the Infinity Cache
    int pair_xcd;  // block->tile map: 0 = batch fastest; LG = 2 / 4 / 8: the LG tiles that share a 128-byte line on one XCD
    cx<T>* h_out;  // RK accumulator write (NULL: == h)
    // per-sample physics (tcfd_ns2d_plan_set_ensemble): {nu, drag, forcing_scale, l00} of the launch's field 0 onwards, or null.  When
    // set, lin / lin_r / lin_c hold the LAPLACIAN (dense, its column 0 and its row 0) and field b steps with
    // L = nu_b * LAP - drag_b (two rounded operations) and forcing_scale_b * forcing; the drivers point it at the chunk's first field
    const T* ens;
    int lsep;      // 1: the linear term in its separable form (== sep on a scalar plan; an ensemble plan tests every member)
};

// fl(fl(nu * lap) - drag): the linear term of one ensemble member, rounded as the element-wise tensor arithmetic that forms
// the (n, m) table of a scalar plan rounds it (no contraction into a fused multiply-add)
template <typename T>
__device__ __forceinline__ T ens_lin(T nu, T lap, T drag) {
#pragma clang fp contract(off)
    const T prod = nu * lap;
    return prod - drag;
}
// forcing_scale * f, rounded once before the sum that takes it
template <typename T>
__device__ __forceinline__ cx<T> ens_force(const cx<T> f, T s) {
#pragma clang fp contract(off)
    return tcfd::mk<T>(f.x * s, f.y * s);
}

// SP = 1 ("split"): the workgroup owns the rows of ONE parity q of the column (i = 2 s + q) and runs N/2-point
// transforms on them; the radix-2 butterfly that joins the two parities rides in the row kernel, which works
// on row pairs (r, r + N/2) anyway.  Workspace rows [0, N/2) then hold the even-part transforms E (resp. the
// folded sums S of the advection), rows [N/2, N) the odd parts O (resp. the twiddled differences D).
// XL = 1 (512-point tiles of 8 columns): the transforms are xl_col_fft512 (one LDS exchange + lane transpositions);
// register t of thread j then holds physical row xl_col_row(j) + t G instead of j + t G.
// The twiddles of a column workgroup's transforms, read ONCE per thread: a MODE_CA workgroup runs five transforms one
// after the other, and a table read inside every pass (behind that pass's barrier) is a memory round trip on its
// dependency chain each time: the s = 0 entry of every pass (tile_fft_rt: the powers come from squaring) for the short
// columns of small grids -- the latency-bound regime -- where the transform shape allows it; else nothing (table reads
// per pass; the long-column kernels sit at their 128-register cap, and the cross-lane tiles read two entries per transform).
template <typename T, int NT, int EPT, int XL>
struct ColTw {
    static constexpr bool RT = !XL && NT <= 256 && is_pow2c(NT) && is_pow2c(EPT) && pass_tw_count<NT, EPT>() > 0 && pass_tw_single<NT, EPT>();
    static constexpr int CNT = RT ? pass_tw_count<NT, EPT>() : 1;
    cx<T> w[CNT];
    __device__ __forceinline__ void load(const cx<T>* __restrict__ tw, int j) {
        if constexpr (RT) load_pass_tw<T, NT, EPT>(w, tw, j);
    }
};
// LDS of a column workgroup behind the exchange tile: the row tables rt_kx, rt_lin, rt_mask (NT reals each), then -- cross-lane
// tiles with table twiddles only -- the XL_COL_TAB_ELEMS stage-two roots.  The kernel, col_fft and the launcher all take the
// layout from here.
constexpr int COL_ROW_TABLES = 3;
template <typename T, int NT, int EPT, int C>
__device__ __forceinline__ T* col_row_tables(cx<T>* lds) { return reinterpret_cast<T*>(lds + lds_elems<NT, EPT, C, false>()); }
template <typename T, int NT, int EPT, int C>
__device__ __forceinline__ cx<T>* col_xl_tab(cx<T>* lds) {
    return reinterpret_cast<cx<T>*>(col_row_tables<T, NT, EPT, C>(lds) + COL_ROW_TABLES * NT);
}
template <typename T, int NT, int EPT, int C>
constexpr size_t col_lds_bytes(bool xl_tab) {
    return (size_t)lds_elems<NT, EPT, C, false>() * sizeof(cx<T>) + COL_ROW_TABLES * (size_t)NT * sizeof(T) +
           (xl_tab ? XL_COL_TAB_ELEMS * sizeof(cx<T>) : 0);
}
template <typename T, int NT, int EPT, int DIR, int C, int XL, int XLT>
__device__ __forceinline__ void col_fft(cx<T> (&x)[EPT], cx<T>* lds, const cx<T>* __restrict__ tw,
                                        const ColTw<T, NT, EPT, XLT>& ctw, int j, int c) {
    if constexpr (XL) {   // two table entries, read per transform: 8 more live registers spill the fp64 kernels
        // (table twiddles: the second entry is the lane's column of the workgroup's stage-two table instead, filled in k_cols)
        const XlColTw<T> t = xl_col_load_tw<T>(tw, j, col_xl_tab<T, NT, EPT, C>(lds));
        xl_col_fft512<T, DIR>(x, lds, t, (int)threadIdx.x);
    } else if constexpr (!XLT && ColTw<T, NT, EPT, XLT>::RT) {
        NoHook nohook;
        tile_fft_rt<T, NT, EPT, DIR, C, false, true>(x, lds, j, c, nohook, ctw.w);
    } else {
        tile_fft<T, NT, EPT, DIR, C, false, true>(x, lds, tw, j, c);
    }
}

// Value of plane f at one spectral element, `u` = w^ (unscaled):
// f=0: u^ = 2 pi i ky psi   f=1: v^ = -2 pi i kx psi   f=2: dx w^ = 2 pi i kx w   f=3: dy w^ = 2 pi i ky w,   all / n^2,
// psi = -w / lap, lap = -4 pi^2 (kx^2 + ky^2), lap(0,0) patched to 1 (`origin`; kx = ky = 0 there, so the value is 0).
// Everything that does not change from element to element is out of the element: 1 / n^2, 2 pi and the signs are the
// compile-time constants P = 1 / (2 pi n^2), S = 2 pi / n^2 (PlaneConst), and the column's factor `kyc` (ky P for plane 0,
// ky S for plane 3: plane_col_const) is formed once per thread and plane.  A plane-0/1 element costs mul + FMA, the
// reciprocal and three or four products, a plane-2/3 element two or three (scaling every element by 1 / n^2, rebuilding lap
// and 2 pi k per element: 12 + the reciprocal, resp. 5); the fp64 plane passes are bound by vector issue.  Nothing is
// carried from plane to plane: the kernels sit at their 128-register cap without scratch, and one more live double spills
// them -- for the same reason -1/lap is formed per plane (eight values across a transform; the 4 KB of LDS a tile has left
// do not hold them).
template <typename T, int N>
struct PlaneConst {
    static constexpr __host__ __device__ T P() { return (T)(0.15915494309189533576888376337251 / ((double)N * (double)N)); }
    static constexpr __host__ __device__ T S() { return (T)(6.283185307179586476925286766559 / ((double)N * (double)N)); }
};
template <typename T, int N>
__device__ __forceinline__ T plane_col_const(int f, T ky) {
    return ky * (f == 0 ? PlaneConst<T, N>::P() : PlaneConst<T, N>::S());
}
template <typename T, int N>
__device__ __forceinline__ cx<T> plane_value(int f, cx<T> u, T kx, T ky, T kyc, bool origin) {
    T c;
    if (f < 2) {
        T d = fma(ky, ky, kx * kx);
        if (origin) d = (T)1;
        c = (f == 0 ? kyc : kx * -PlaneConst<T, N>::P()) * fast_rcp(d);
    } else {
        c = f == 2 ? kx * PlaneConst<T, N>::S() : kyc;
    }
    return mk<T>(-u.y * c, u.x * c);
}

// PACKED NYQUIST COLUMN (a.nyq).  m = n/2 + 1 columns are n/2 / C full tiles plus ONE lone column, whose tile costs a
// whole workgroup: with 4 fields of 1024^2 per chunk that makes 520 workgroups for the 512 resident slots, and the
// 8 late ones stretch every launch by most of a workgroup's run time (measured: MODE_A 54 -> 39 us without them).
// The row pass consumes only the REAL parts of columns 0 and m - 1 of a plane (c2r semantics: Im of the DC and
// Nyquist coefficients of a row is dropped).  Re(IFFT(A)) = IFFT(herm A), herm A[k] = (A[k] + conj A[-k]) / 2, so
// both columns ride through ONE transform,
//     Z = herm(A_0) + i herm(A_nyq)   ->   IFFT(Z) = Re(IFFT A_0) + i Re(IFFT A_nyq),
// stored in column 0: the row pass takes its Nyquist element from the imaginary part of element 0.  (With the split
// plans the same holds per parity: the E / O half transforms and the row pass's butterfly are complex-linear.)
// Tile 0 builds Z through the exchange buffer (free between two transforms), one row per thread of the workgroup.
// The Nyquist column's own values wait in LDS (`un`: the rt_lin / rt_mask tables are dead by then and exactly that
// big): registers held across the four transforms would spill the fp64 kernels.
template <typename T, int N, int EPT, int C, int SP, int XL>
__device__ __forceinline__ void emit_planes(const ColArgs<T>& a, const cx<T> (&u)[EPT], cx<T>* lds, const T* rt_kx,
                                            size_t wbase, int j, int c, int jc, bool valid, int q,
                                            const ColTw<T, (N >> SP), EPT, XL>& ctw, bool nyq_tile, const cx<T>* un) {
    constexpr int NT = N >> SP;
    constexpr int G = NT / EPT;
    const T ky = valid ? a.ky[jc] : (T)0;
    const bool nyq_lane = nyq_tile && c == 0;
    const T ky_n = nyq_tile ? a.ky[a.m - 1] : (T)0;
#pragma unroll 1
    for (int f = 0; f < 4; ++f) {
        cx<T> x[EPT];
        const T kyc = plane_col_const<T, N>(f, ky);
#pragma unroll
        for (int t = 0; t < EPT; ++t) {
            const int sl = j + t * G;
            const int i = SP ? 2 * sl + q : sl;
            const cx<T> v = plane_value<T, N>(f, u[t], rt_kx[sl], ky, kyc, i == 0 && jc == 0);
            x[t] = valid ? v : mk<T>((T)0, (T)0);
        }
        if (nyq_tile && !(a.ablate & 64)) {   // block-uniform.  Three short phases with the WHOLE workgroup (a row per thread), so that
            cx<T>* S0 = lds;           // tile 0 does not become the launch's long pole
            cx<T>* SZ = lds + NT;
            if (nyq_lane) {
#pragma unroll
                for (int t = 0; t < EPT; ++t) S0[j + t * G] = x[t];
            }
            __syncthreads();
            for (int sl = threadIdx.x; sl < NT; sl += C * G) {
                // row -i of the column: local index of the same parity
                const int ms = (SP && q) ? NT - 1 - sl : (NT - sl) % NT;
                const cx<T> v0 = S0[sl], m0 = S0[ms];
                const T kyc_n = plane_col_const<T, N>(f, ky_n);
                const cx<T> vn = plane_value<T, N>(f, un[sl], rt_kx[sl], ky_n, kyc_n, false);
                const cx<T> mn = plane_value<T, N>(f, un[ms], rt_kx[ms], ky_n, kyc_n, false);
                const cx<T> h0 = mk<T>((T)0.5 * (v0.x + m0.x), (T)0.5 * (v0.y - m0.y));
                const cx<T> hn = mk<T>((T)0.5 * (vn.x + mn.x), (T)0.5 * (vn.y - mn.y));
                SZ[sl] = mk<T>(h0.x - hn.y, h0.y + hn.x);   // h0 + i hn
            }
            __syncthreads();
            if (nyq_lane) {
#pragma unroll
                for (int t = 0; t < EPT; ++t) x[t] = SZ[j + t * G];
            }
            __syncthreads();
        }
        const int jrow = XL ? xl_col_row(j) : j;   // physical row (mod G) of this thread's outputs
        if (!(a.ablate & 1)) col_fft<T, NT, EPT, +1, C, XL, XL>(x, lds, a.tw, ctw, j, c);
        if (valid && !(a.ablate & 2)) {
            cx<T>* dst = a.planes + (size_t)f * a.plane_stride + wbase + (size_t)(SP ? q * NT : 0) * a.ldw;
            if (a.nt_planes) {
#pragma unroll
                for (int t = 0; t < EPT; ++t) store_stream(dst + (size_t)(jrow + t * G) * a.ldw, x[t]);
            } else {
#pragma unroll
                for (int t = 0; t < EPT; ++t) dst[(size_t)(jrow + t * G) * a.ldw] = x[t];
            }
        }
    }
}

// x[t] (column FFT of the advection) -> F = mask * x + forcing, in place (equations.py:424-437)
template <typename T, int N, int EPT, int SP, int ENS>
__device__ __forceinline__ void apply_mask_forcing(const ColArgs<T>& a, cx<T> (&x)[EPT], int j, int jc,
                                                   const T* rt_mask, T cm, int f_lo, int f_hi, int q, T fs) {
    constexpr int G = (N >> SP) / EPT;
    // ENS: the member's forcing is fs * forcing (fs is workgroup-uniform)
#define TCFD_IROW(t_) (SP ? 2 * (j + (t_) * G) + q : j + (t_) * G)
    if (a.ablate & 4) return;
    if (a.sep) {
#pragma unroll
        for (int t = 0; t < EPT; ++t) x[t] = cscale(x[t], rt_mask[j + t * G] * cm);
    } else {
#pragma unroll
        for (int t = 0; t < EPT; ++t) x[t] = cscale(x[t], a.mask[(size_t)TCFD_IROW(t) * a.m + jc]);
    }
    if (a.f_nnz > 0) {  // a handful of entries in total (1 for Kolmogorov forcing): uniform loop
        for (int e = 0; e < a.f_nnz; ++e) {
            const int r = a.f_row[e];
            const int fc = a.f_col[e];      // all three reads of an entry before the branch: one round trip, not two
            cx<T> v = a.f_val[e];
            if constexpr (ENS) v = ens_force(v, fs);
            if (fc == jc) {
#pragma unroll
                for (int t = 0; t < EPT; ++t)
                    if (r == TCFD_IROW(t)) x[t] = x[t] + v;
            }
        }
    } else if (a.f_ptr) {  // sparse, many entries: this column's slice of the CSC list
        for (int e = f_lo; e < f_hi; ++e) {
            const int r = a.f_row[e];
            cx<T> v = a.f_val[e];
            if constexpr (ENS) v = ens_force(v, fs);
#pragma unroll
            for (int t = 0; t < EPT; ++t)
                if (r == TCFD_IROW(t)) x[t] = x[t] + v;
        }
    } else if (a.forcing) {
#pragma unroll
        for (int t = 0; t < EPT; ++t) {
            cx<T> v = a.forcing[(size_t)TCFD_IROW(t) * a.m + jc];
            if constexpr (ENS) v = ens_force(v, fs);
            x[t] = x[t] + v;
        }
    }
#undef TCFD_IROW
}

// NYQ = 1: the variant that can run with a.nyq (packed Nyquist column); kept apart because the extra code costs the
// register-capped fp64 kernels a few spilled registers in EVERY workgroup, packed or not
// ENS = 1: per-sample physics (a.ens is set; MODE_CA / C / F / RES).  Its own instantiations for the same reason: as a
// workgroup-uniform branch the member arithmetic moved the register count of most scalar kernels and cost several of them a wave
// of occupancy (profiles/ns2d_ensemble_kernel_resource_usage.txt); with ENS = 0 the kernel is the one it was
template <typename T, int N, int EPT, int C, int MODE, int MINW, int SP = 0, int XL = 0, int NYQ = 0, int ENS = 0>
__global__ __launch_bounds__(C*((N >> SP) / EPT), MINW) void k_cols(ColArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw);
    constexpr int NT = N >> SP;  // transform length (half the column when the workgroup owns one parity)
    constexpr int G = NT / EPT;
    static_assert(!(SP && (MODE == MODE_FWD || MODE == MODE_INV)), "plain transforms are not split");
    // parity of the spectral rows this workgroup owns: the LOW bit of the block id, so that the two parity workgroups
    // of a tile are dispatched next to each other -- to different XCDs.  (As blockIdx.y they were 256 ids apart, i.e.
    // in the two slots of ONE CU: with the packed Nyquist column both long workgroups of tile 0 shared that CU.)
    const int q = SP ? (int)(blockIdx.x & 1) : 0;
    const unsigned bx = SP ? blockIdx.x >> 1 : blockIdx.x;
#define TCFD_IROW(s_) (SP ? 2 * (s_) + q : (s_))
    const size_t wq = (size_t)(SP ? q * NT : 0);  // first workspace row of this parity
    const int c = threadIdx.x % C;
    const int j = threadIdx.x / C;
    // batch is the fastest block index: the blocks that share one tile of the (n, m) tables
    // (linear term, mask, forcing) run together and hit them in L2
    int tile;
    long b;
    if (a.pair_xcd) {
        // tiles narrower than a 128-byte line: the LG = 2 or 4 tiles that share a line are issued 8 block ids apart,
        // i.e. on the SAME XCD (block id % 8): their partial-line stores merge in that XCD's L2 into whole dirty
        // lines before the end-of-kernel write-back (each XCD writing its own 32 bytes of a line costs a fabric
        // transaction per piece: the plane stores were 7 of the 17 us of a 256^2 x 16 column pass)
        const unsigned LG = (unsigned)a.pair_xcd, span = 8 * LG;
        const unsigned q = bx / span, r = bx % span;
        const unsigned unit = q * 8 + (r % 8);
        if (unit >= (unsigned)(((a.ntiles + LG - 1) / LG) * a.batch)) return;
        tile = (int)(LG * (unit / a.batch) + r / 8);
        b = unit % a.batch;
    } else {
        tile = bx / a.batch;
        b = bx % a.batch;
    }
    const int jc = tile * C + c;
    const bool valid = jc < a.m;
    // the member's {nu, drag, forcing scale}: b is workgroup-uniform, so these are three uniform loads into scalar registers
    // (and l00 = nu * LAP[0][0] - drag, which the host formed with the same two roundings: no dependent load for it here)
    [[maybe_unused]] T e_nu = 1, e_drag = 0, e_fs = 1, e_l00 = 0;
    if constexpr (ENS) {
        const T* e = a.ens + 4 * (size_t)b;
        e_nu = e[0]; e_drag = e[1]; e_fs = e[2]; e_l00 = e[3];
    }
    // the linear term from a table entry: the entry itself, or (ensemble) the member's nu * laplacian - drag
    [[maybe_unused]] auto lin_of = [&](T raw) -> T {
        if constexpr (ENS) return ens_lin(e_nu, raw, e_drag);
        else return raw;
    };
    const int lsep = ENS ? a.lsep : a.sep;   // (a scalar plan: one flag for the mask and the linear term)
    const bool nyq_tile = NYQ && a.nyq && tile == 0;   // block-uniform: the lanes c == 0 of this workgroup also own column m - 1
    const bool nyq_lane = nyq_tile && c == 0;
    const size_t colbase = (size_t)b * N * a.m + jc;   // element (b, 0, jc) of a caller-layout array
    const size_t wbase = (size_t)b * N * a.ldw + jc;   // same element of a workspace array

    // per-row constants (kx, separable parts of the linear term and of the mask) live in LDS behind the
    // exchange tile: every later use is an LDS read instead of a dependent global load; per-column
    // constants and the forcing column range are fetched up front, before the transform needs them
    T* rt_kx = col_row_tables<T, NT, EPT, C>(lds);
    T* rt_lin = rt_kx + NT;
    T* rt_mask = rt_lin + NT;
    cx<T>* un_lds = reinterpret_cast<cx<T>*>(rt_lin);   // [NT]: Nyquist-column state (a.nyq), overlays rt_lin + rt_mask
    constexpr bool NEEDS_TABLES = (MODE != MODE_FWD && MODE != MODE_INV);
    T col_ky = 0, col_lin = 0, col_mask = 1;
    int f_lo = 0, f_hi = 0;
    // Called AFTER the tile's own loads have been issued: the table reads (three loads whose results go to LDS, in a
    // loop the compiler does not move loads across) then ride in the shadow of the tile's memory round trip instead
    // of adding two of their own in front of it.  The null tables of a non-separable plan are read through `kx`.
    // (XL_TAB instantiations of the transforming modes: the barrier that makes the tables visible stands in FRONT of the
    // first transform, which twiddles from LDS before its own first barrier -- there the table reads are waited for with
    // the tile's loads instead of behind the transform.)
    auto stage_tables = [&]() {
        if constexpr (NEEDS_TABLES) {
            const T* lin_r = lsep ? a.lin_r : a.kx;
            const T* mask_r = a.sep ? a.mask_r : a.kx;
            // ensemble: lin_r[i] + lin_c[j] of the member, formed from the laplacian's column 0 and row 0 as plan_fill forms a
            // scalar plan's pair from its table (lin_r[i] = l[i][0] - l[0][0], lin_c[j] = l[0][j]): the same bits
            for (int sl = threadIdx.x; sl < NT; sl += C * G) {  // indexed by the LOCAL row sl, spectral row IROW(sl)
                const int i = TCFD_IROW(sl);
                const T vk = a.kx[i], vl = lin_r[i], vm = mask_r[i];
                rt_kx[sl] = vk;
                if constexpr (ENS) rt_lin[sl] = lsep ? ens_lin(e_nu, vl, e_drag) - e_l00 : (T)0;
                else rt_lin[sl] = a.sep ? vl : (T)0;
                rt_mask[sl] = a.sep ? vm : (T)1;
            }
            if (valid) {
                col_ky = a.ky[jc];
                if constexpr (ENS) {
                    // the laplacian's entry as loaded; lin_of is applied where L is formed: arithmetic on the value HERE makes
                    // the wave wait for this load -- and for the tile's loads issued before it -- ahead of the loads that follow
                    if (lsep) col_lin = a.lin_c[jc];
                    if (a.sep) col_mask = a.mask_c[jc];
                } else {
                    if (a.sep) { col_lin = a.lin_c[jc]; col_mask = a.mask_c[jc]; }
                }
                if (a.f_ptr && a.f_nnz == 0) { f_lo = a.f_ptr[jc]; f_hi = a.f_ptr[jc + 1]; }
            }
        }
    };

    ColTw<T, NT, EPT, XL> ctw;
    ctw.load(a.tw, j);
    // cross-lane tiles with table twiddles: the 8 x 8 roots of the second stage, behind the row tables; its read goes out ahead
    // of the tile's own, and the first barrier below makes it visible
    constexpr bool XL_TAB = XL && xl_col_direct<T>();
    if constexpr (XL_TAB) xl_col_fill_tab<T>(col_xl_tab<T, NT, EPT, C>(lds), a.tw, (int)threadIdx.x);
    cx<T> x[EPT];
    if constexpr (MODE == MODE_A) {
        {
            const size_t ub = (size_t)b * N * a.u_in_ld + jc;
#pragma unroll
            for (int t = 0; t < EPT; ++t)
                x[t] = valid ? a.u_in[ub + (size_t)TCFD_IROW(j + t * G) * a.u_in_ld] : mk<T>((T)0, (T)0);
        }
        stage_tables();
        __syncthreads();  // row tables visible
        if (nyq_tile) {   // rt_lin / rt_mask are not used in this mode; visible after the first barrier of emit_planes
            const cx<T>* uin = a.u_in + (size_t)b * N * a.u_in_ld + (a.m - 1);
            for (int sl = threadIdx.x; sl < NT; sl += C * G) un_lds[sl] = uin[(size_t)TCFD_IROW(sl) * a.u_in_ld];
        }
        emit_planes<T, N, EPT, C, SP, XL>(a, x, lds, rt_kx, wbase, j, c, jc, valid, q, ctw, nyq_tile, un_lds);
        return;
    } else {
        constexpr bool GENERIC = (MODE == MODE_FWD || MODE == MODE_INV);
        const int in_ld = GENERIC ? a.in_ld : a.ldw;
        const size_t inbase = (size_t)b * N * in_ld + jc;
        // pruned plans never write the advection for columns >= keep_cols: they are exact zeros
        const bool col_live = valid && (GENERIC || a.keep_cols == 0 || jc < a.keep_cols);
        const bool tile_live = GENERIC || a.keep_cols == 0 || tile * C < a.keep_cols;  // block-uniform
        constexpr int DIR = (MODE == MODE_INV) ? +1 : -1;
        constexpr bool XLF = XL && !GENERIC;   // forward transform of the advection: physical rows come in at xl_col_row
        const int jin = XLF ? xl_col_row(j) : j;
#pragma unroll
        for (int t = 0; t < EPT; ++t)
            x[t] = col_live ? TCFD_COL_LD(a.in + inbase + (wq + (size_t)(jin + t * G)) * in_ld) : mk<T>((T)0, (T)0);
        stage_tables();
        if constexpr (XL_TAB) __syncthreads();   // this transform twiddles from the table before its first barrier; row tables visible too
        if (!(a.ablate & 1) && tile_live) col_fft<T, NT, EPT, DIR, C, XLF ? 1 : 0, XL>(x, lds, a.tw, ctw, j, c);
        if constexpr (NEEDS_TABLES && !XL_TAB) __syncthreads();  // row tables visible (a one-pass transform has no barrier)

        if constexpr (MODE == MODE_FWD || MODE == MODE_INV) {
            if (valid) {
                const size_t outbase = (size_t)b * N * a.out_ld + jc;
#pragma unroll
                for (int t = 0; t < EPT; ++t) a.out[outbase + (size_t)(j + t * G) * a.out_ld] = cscale(x[t], a.scale);
            }
            return;
        } else if constexpr (MODE == MODE_F) {
            if (valid) {
                apply_mask_forcing<T, N, EPT, SP, ENS>(a, x, j, jc, rt_mask, col_mask, f_lo, f_hi, q, e_fs);
#pragma unroll
                for (int t = 0; t < EPT; ++t) a.out[colbase + (size_t)TCFD_IROW(j + t * G) * a.m] = x[t];
            }
            return;
        } else if constexpr (MODE == MODE_RES) {
            if (valid) {
                constexpr T M4PI2 = (T)(-39.478417604357434475337963999505);
                const T ky = col_ky;
                apply_mask_forcing<T, N, EPT, SP, ENS>(a, x, j, jc, rt_mask, col_mask, f_lo, f_hi, q, e_fs);
                const T lc = lin_of(col_lin);
#pragma unroll
                for (int t = 0; t < EPT; ++t) {
                    const int sl = j + t * G;
                    const int i = TCFD_IROW(sl);
                    const size_t g = colbase + (size_t)i * a.m;
                    const cx<T> F = x[t];
                    const cx<T> w = a.u_in[g];
                    if (a.out) {
                        const cx<T> wt = a.wt[g];
                        const T L = lsep ? rt_lin[sl] + lc : lin_of(a.lin[(size_t)i * a.m + jc]);
                        a.out[g] = wt - F - cscale(w, L);
                    }
                    if (a.psi) {
                        const T kx = rt_kx[sl];
                        T lap = M4PI2 * (kx * kx + ky * ky);
                        if (i == 0 && jc == 0) lap = (T)1;
                        a.psi[g] = cscale(w, (T)-1 / lap);
                    }
                }
            }
            return;
        } else {  // MODE_CA / MODE_C : Runge-Kutta accumulate + Crank-Nicolson solve
            constexpr bool writer = true;
            // packed Nyquist column (tile 0, a row per thread): its reads go out first, in the shadow of the tile's own
            constexpr int NYQ_PER = (NT + C * G - 1) / (C * G);
            [[maybe_unused]] cx<T> nyq_u[NYQ_PER], nyq_w0[NYQ_PER];
            if (nyq_tile) {
#pragma unroll
                for (int r = 0; r < NYQ_PER; ++r) {
                    const int sl = threadIdx.x + r * C * G;
                    if (sl < NT) {
                        const int i = TCFD_IROW(sl);
                        nyq_u[r] = a.u_in[(size_t)b * N * a.u_in_ld + (a.m - 1) + (size_t)i * a.u_in_ld];
                        if constexpr (MODE == MODE_C) {
                            if (a.dwdt) nyq_w0[r] = a.w0[(size_t)b * N * a.m + (a.m - 1) + (size_t)i * a.m];
                        }
                    }
                }
            }
            if (valid) {
                // Every global read of the update is issued before the first value is used: the reads of one thread
                // are independent, but `h` and the state are updated in place through pointers that may alias, so
                // a load written after an earlier element's store is not moved above it -- 2 EPT memory round trips
                // one after the other.  In the cache-resident regimes (chunked 1024^2, small grids) a workgroup's
                // dependency chain IS the kernel time.
                const T lc = lin_of(col_lin);
                const size_t ub = (size_t)b * N * a.u_in_ld + jc;
                apply_mask_forcing<T, N, EPT, SP, ENS>(a, x, j, jc, rt_mask, col_mask, f_lo, f_hi, q, e_fs);
                // UB elements per batch of reads: everything at once where the registers are there (fp32, short
                // columns), 64 bytes' worth per array otherwise (the long-column kernels sit at the 128-register cap)
                constexpr int UB = EPT * (int)sizeof(cx<T>) <= 64 ? EPT : 64 / (int)sizeof(cx<T>);   // 8 fp32 / 4 fp64
#pragma unroll
                for (int t0 = 0; t0 < EPT; t0 += UB) {
                    cx<T> hv[UB], uv[UB];
                    [[maybe_unused]] cx<T> w0v[UB];
                    T Lv[UB];
                    bool h_live[UB];
#pragma unroll
                    for (int tt = 0; tt < UB; ++tt) {
                        const int sl = j + (t0 + tt) * G;
                        const int i = TCFD_IROW(sl);
                        // pruned entries: F = 0 at every stage, so h stays 0 and is not stored at all
                        h_live[tt] = !(a.ablate & 8) && (a.keep_cols == 0 || (col_live && rt_mask[sl] != (T)0));
                        hv[tt] = (h_live[tt] && a.load_h) ? a.h[wbase + (wq + (size_t)sl) * a.ldw] : mk<T>((T)0, (T)0);
                        uv[tt] = a.u_in[ub + (size_t)i * a.u_in_ld];
                        Lv[tt] = (a.ablate & 4) ? (T)-0.5 : (lsep ? rt_lin[sl] + lc : lin_of(a.lin[(size_t)i * a.m + jc]));
                        if constexpr (MODE == MODE_C) {
                            if (a.dwdt) w0v[tt] = a.w0[(size_t)b * N * a.m + jc + (size_t)i * a.m];
                        }
                    }
#pragma unroll
                    for (int tt = 0; tt < UB; ++tt) {
                        const int t = t0 + tt;
                        const int sl = j + t * G;
                        const int i = TCFD_IROW(sl);
                        const size_t gw = wbase + (wq + (size_t)sl) * a.ldw;  // h is stored parity-major when split
                        const cx<T> hn = cscale(x[t], a.fa) + cscale(hv[tt], a.beta);   // hv = 0: nothing to add
                        if (h_live[tt] && a.store_h && writer) a.h_out[gw] = hn;
                        const T L = Lv[tt];
                        const cx<T> u = uv[tt];
                        // u + gamma dt h + mu L u, then / (1 - mu L)     (equations.py:355-357)
                        cx<T> rhs = u + cscale(hn, a.gdt) + cscale(cscale(u, L), a.mu);
                        const T den = fast_rcp((T)1 - a.mud * L);
                        x[t] = cscale(rhs, den);
                        if constexpr (MODE == MODE_C) {
                            cx<T>* const po = a.u_out + (size_t)b * N * a.u_out_ld + jc + (size_t)i * a.u_out_ld;
                            if (writer) {
                                if (a.nt_out) store_stream(po, x[t]);
                                else *po = x[t];
                            }
                            if (a.dwdt) {   // (w_new - w_old) / (steps dt), equations.py:461-462, fused into the last stage
                                const size_t gi = (size_t)b * N * a.m + jc + (size_t)i * a.m;
                                const cx<T> dv = cscale(x[t] - w0v[tt], a.dwdt_scale);
                                if (a.nt_out) store_stream(a.dwdt + gi, dv);
                                else a.dwdt[gi] = dv;
                            }
                        } else {
                            if (writer) a.u_out[(size_t)b * N * a.u_out_ld + jc + (size_t)i * a.u_out_ld] = x[t];
                        }
                    }
                }
            }
            if (nyq_tile && !(a.ablate & 128)) {   // block-uniform
                // column m - 1, a row per thread: F = 0 there (the plan is pruned: keep_cols <= m - 1), so h stays 0 and
                // the stage is  u <- (u + mu L u) / (1 - mud L)
                const int jn = a.m - 1;
                const T lcn = lsep ? lin_of(a.lin_c[jn]) : (T)0;
                constexpr int PER = NYQ_PER;
                cx<T> unew[PER];
#pragma unroll
                for (int r = 0; r < PER; ++r) {
                    const int sl = threadIdx.x + r * C * G;
                    if (sl < NT) {
                        const int i = TCFD_IROW(sl);
                        const cx<T> uo = nyq_u[r];
                        const T L = (a.ablate & 4) ? (T)-0.5 : (lsep ? rt_lin[sl] + lcn : lin_of(a.lin[(size_t)i * a.m + jn]));
                        const cx<T> rhs = uo + cscale(cscale(uo, L), a.mu);
                        unew[r] = cscale(rhs, fast_rcp((T)1 - a.mud * L));
                        if (writer) a.u_out[(size_t)b * N * a.u_out_ld + jn + (size_t)i * a.u_out_ld] = unew[r];
                        if constexpr (MODE == MODE_C) {
                            if (a.dwdt) {
                                const size_t gi = (size_t)b * N * a.m + jn + (size_t)i * a.m;
                                a.dwdt[gi] = cscale(unew[r] - nyq_w0[r], a.dwdt_scale);
                            }
                        }
                    }
                }
                if constexpr (MODE == MODE_CA) {
                    __syncthreads();   // every lane is done with rt_lin / rt_mask: the Nyquist column moves in
#pragma unroll
                    for (int r = 0; r < PER; ++r) {
                        const int sl = threadIdx.x + r * C * G;
                        if (sl < NT) un_lds[sl] = unew[r];
                    }
                }
            }
            if constexpr (MODE == MODE_CA)
                emit_planes<T, N, EPT, C, SP, XL>(a, x, lds, rt_kx, wbase, j, c, jc, valid, q, ctw, nyq_tile, un_lds);
        }
    }
#undef TCFD_IROW
}

// ------------------------------------------------------------------ row kernels
// One group of G lanes owns one PAIR of adjacent rows: two real rows ride through
// one complex transform (x0 + i x1), so c2r/r2c cost one complex FFT per two rows.

// Hermitian-extended load of the pair (A row, B row): sequence Z[e] = A~[e] + i B~[e]
// where A~ is the Hermitian completion of the half row with Im(DC), Im(Nyquist)
// dropped -- exactly what a c2r transform consumes (SURVEY note N2).
template <typename T, int N, int EPT>
__device__ __forceinline__ void load_herm_pair(cx<T> (&x)[EPT], const cx<T>* __restrict__ rowA,
                                               const cx<T>* __restrict__ rowB, int j) {
    constexpr int G = N / EPT;
#pragma unroll
    for (int t = 0; t < EPT; ++t) {
        const int e = j + t * G;
        if (t < EPT / 2) {
            cx<T> pa = rowA[e], pb = rowB[e];
            if (e == 0) { pa.y = 0; pb.y = 0; }
            x[t] = mk<T>(pa.x - pb.y, pa.y + pb.x);
        } else {
            const int k = N - e;  // 1 .. N/2
            cx<T> pa = rowA[k], pb = rowB[k];
            if (k == N / 2) { pa.y = 0; pb.y = 0; }
            // conj(a) + i conj(b)
            x[t] = mk<T>(pa.x + pb.y, pb.x - pa.y);
        }
    }
}

// x holds Z = FFT(r0 + i r1) distributed j + t*G; writes the half spectra of r0, r1.
template <typename T, int N, int EPT>
__device__ __forceinline__ void unpack_store_pair(const cx<T> (&x)[EPT], cx<T>* lds, cx<T>* __restrict__ out0,
                                                  cx<T>* __restrict__ out1, int j, bool valid, int kc = N) {
    constexpr int G = N / EPT;
    constexpr bool WG = (G > 64);
#pragma unroll
    for (int t = 0; t < EPT; ++t) lds[lds_addr<EPT, 1, true>(j + t * G, 0)] = x[t];
    group_sync<WG>();
    const T half = (T)0.5;
#pragma unroll
    for (int t = 0; t < EPT / 2; ++t) {
        const int k = j + t * G;
        const cx<T> A = x[t];
        const cx<T> Bm = lds[lds_addr<EPT, 1, true>((N - k) % N, 0)];
        const cx<T> S = mk<T>(A.x + Bm.x, A.y - Bm.y);  // A + conj(B) = 2 X0
        const cx<T> D = mk<T>(A.x - Bm.x, A.y + Bm.y);  // A - conj(B) = 2 i X1
        if (valid && k < kc) {  // kc: columns the consumer reads (2/3-rule pruning)
            out0[k] = cscale(S, half);
            out1[k] = mk<T>(D.y * half, -D.x * half);
        }
    }
    if (j == 0) {
        const cx<T> A = x[EPT / 2];  // element N/2
        if (valid && N / 2 < kc) {
            out0[N / 2] = mk<T>(A.x, (T)0);
            out1[N / 2] = mk<T>(A.y, (T)0);
        }
    }
    group_sync<WG>();
}

template <typename T, int N, int EPT, int THREADS_ = 256>
struct RowGeom {
    static constexpr int G = N / EPT;
    static constexpr int THREADS = G >= THREADS_ ? G : THREADS_;
    static constexpr int GROUPS = THREADS / G;
    static constexpr int LDS_PER_GROUP = lds_elems<N, EPT, 1, true>();
    static constexpr size_t LDS_BYTES = (size_t)GROUPS * LDS_PER_GROUP * sizeof(cx<T>);
};

// ---- row pass, software-pipelined ("v3") -------------------------------------------------
// The un-mirrored half rows of two planes as they come from HBM: k = j + G*t, t < EPT/2, plus the
// Nyquist element.  A group keeps TWO of these in registers: the one being consumed and the one in
// flight, so a load phase is never exposed (the plain kernel above alternates load and transform
// phases and reaches only ~3 TB/s at 1024^2).
template <typename T, int EPT>
struct RawPair {
    cx<T> a[EPT / 2], b[EPT / 2];
    cx<T> an, bn;  // element N/2 of both rows (only lane 0 of the group uses it)
};

// nyq (packed Nyquist column, see emit_planes): column N/2 of the planes is not there; the Nyquist element of a row
// is the imaginary part of its element 0 and comes out of pack_herm
// TCFD_NT_ROW_LOADS=1 (build time): the planes a row pass reads are read exactly once by that launch -- non-temporal loads
#ifndef TCFD_NT_ROW_LOADS
#define TCFD_NT_ROW_LOADS 0
#endif
#if TCFD_NT_ROW_LOADS
#define TCFD_ROW_LD(p_) load_stream(p_)
#else
#define TCFD_ROW_LD(p_) (*(p_))
#endif
template <typename T, int N, int EPT, int NYQ = 0>
__device__ __forceinline__ void load_raw(RawPair<T, EPT>& r, const cx<T>* __restrict__ rowA,
                                         const cx<T>* __restrict__ rowB, int j) {
    constexpr int G = N / EPT;
#pragma unroll
    for (int t = 0; t < EPT / 2; ++t) {
        r.a[t] = TCFD_ROW_LD(rowA + j + t * G);
        r.b[t] = TCFD_ROW_LD(rowB + j + t * G);
    }
    if constexpr (!NYQ) {
        r.an = rowA[N / 2];
        r.bn = rowB[N / 2];
    }
}

// Z[e] = A~[e] + i B~[e] (Hermitian completions, Im of DC / Nyquist dropped) in the j + t*G
// distribution.  The upper half is the mirror image of data owned by OTHER lanes: it goes through
// the group's LDS buffer (half an exchange) instead of being loaded from HBM a second time.
// SWZ: the XOR swizzle of the Stockham exchanges (lds_addr<.., true>).  The cross-lane row kernel (v7) has no stride-EPT
// stores -- its transform exchanges through xl_slot -- and passes SWZ = false: with the swizzle the MIRRORED accesses
// (lanes j -> slots N - j, descending) straddle two 8-element blocks with different XOR constants and collide pairwise
// (rocprofv3: SQ_LDS_BANK_CONFLICT 0.84 M of 4.03 M LDS-array cycles per chunk launch); unswizzled, descending consecutive
// 16-byte slots are conflict free for both the 8-lane store groups and the 16-lane load groups of the b128 instructions.
template <typename T, int N, int EPT, bool WG, int NYQ = 0, bool SWZ = true>
__device__ __forceinline__ void pack_herm(cx<T> (&x)[EPT], const RawPair<T, EPT>& r, cx<T>* lds, int j) {
    constexpr int G = N / EPT;
    // G % EPT^2 == 0: the swizzle term of lds_addr is the same for every t, so the mirrored slots N - j - t G and
    // the read slots j + t G are ONE address each plus compile-time offsets
    constexpr bool AFFINE = !SWZ || (G % (EPT * EPT) == 0);
    cx<T>* mir = lds + lds_addr<EPT, 1, SWZ>(N - j, 0);   // j = 0: slot N is never touched (k >= 1 below)
#pragma unroll
    for (int t = 0; t < EPT / 2; ++t) {
        const int k = j + t * G;
        cx<T> pa = r.a[t], pb = r.b[t];
        if (k == 0) { pa.y = 0; pb.y = 0; }
        x[t] = mk<T>(pa.x - pb.y, pa.y + pb.x);
        if (k >= 1) {
            const cx<T> m = mk<T>(pa.x + pb.y, pb.x - pa.y);
            if constexpr (AFFINE) mir[-t * G] = m;
            else lds[lds_addr<EPT, 1, SWZ>(N - k, 0)] = m;
        }
    }
    if (j == 0)   // lane 0 holds element 0 in a[0] / b[0]
        lds[lds_addr<EPT, 1, SWZ>(N / 2, 0)] = NYQ ? mk<T>(r.a[0].y, r.b[0].y) : mk<T>(r.an.x, r.bn.x);
    group_sync<WG>();
    const cx<T>* src = lds + lds_addr<EPT, 1, SWZ>(j, 0);
#pragma unroll
    for (int t = EPT / 2; t < EPT; ++t) {
        if constexpr (AFFINE) x[t] = src[t * G];
        else x[t] = lds[lds_addr<EPT, 1, SWZ>(j + t * G, 0)];
    }
    group_sync<WG>();
}

// ---- row pass of the VECTOR-JACOBIAN PRODUCT of the explicit terms -----------------------------------------------
// F(w) = M . R( -(dxw u + dyw v) ) [+ f],  u, v, dxw, dyw = I(a_f w).  For a cotangent g:  nbar = R^T(M g) is a real field
// (plane 4 holds the column-transformed M g / c), and the cotangents of the four inverse transforms are nbar times the
// PARTNER of each factor:   Y0 = nbar dxw (-> u^),  Y1 = nbar dyw (-> v^),  Y2 = nbar u (-> dxw^),  Y3 = nbar v (-> dyw^).
// One group per row pair, two rows per complex transform as in v5: five c2r, four products, four r2c; the Y rows replace
// the plane rows they were computed from (a pair's rows belong to its group alone).  Plain (non-split) plane layout.
template <typename T, int N, int EPT, int THR>
__global__ __launch_bounds__((RowGeom<T, N, EPT, THR>::THREADS)) void k_rows_vjp(cx<T>* __restrict__ planes, size_t plane_stride,
                                                                                 const cx<T>* __restrict__ gplane,
                                                                                 const cx<T>* __restrict__ tw, long npairs, int ld) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT, THR>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    const long stride = (long)gridDim.x * Gm::GROUPS;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const long iters = (npairs + stride - 1) / stride;   // every group runs the same number of iterations (workgroup barriers)
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const size_t off = (size_t)cur * 2 * (size_t)ld;
        RawPair<T, EPT> H;
        auto field = [&](cx<T>(&out)[EPT], const cx<T>* rowA) {
            load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
            pack_herm<T, N, EPT, WG>(out, H, lds, j);
            tile_fft<T, N, EPT, +1, 1, true, WG>(out, lds, tw, j, 0);
        };
        auto emit = [&](const cx<T>(&nb)[EPT], const cx<T>(&fld)[EPT], cx<T>* rowA) {
            cx<T> y[EPT];
#pragma unroll
            for (int t = 0; t < EPT; ++t) y[t] = mk<T>(nb[t].x * fld[t].x, nb[t].y * fld[t].y);
            tile_fft<T, N, EPT, -1, 1, true, WG>(y, lds, tw, j, 0);
            unpack_store_pair<T, N, EPT>(y, lds, rowA, rowA + ld, j, valid);
        };
        cx<T> nb[EPT], fa[EPT], fb[EPT];
        cx<T>* P0 = planes + off;
        cx<T>* P1 = planes + plane_stride + off;
        cx<T>* P2 = planes + 2 * plane_stride + off;
        cx<T>* P3 = planes + 3 * plane_stride + off;
        field(nb, gplane + off);
        field(fa, P2);          // dx w
        field(fb, P0);          // u
        emit(nb, fa, P0);       // Y0 = nbar dxw
        emit(nb, fb, P2);       // Y2 = nbar u
        field(fa, P3);          // dy w
        field(fb, P1);          // v
        emit(nb, fa, P1);       // Y1 = nbar dyw
        emit(nb, fb, P3);       // Y3 = nbar v
    }
}

// ---- row pass of the JACOBIAN-VECTOR PRODUCT (tangent-linear model) of the explicit terms ---------------------------------
// A state w and a perturbation dw ride through the advection together:  with the four planes of w (`planes`) and of dw
// (`dplanes`, same layout),
//     p  = -(u dxw + v dyw)                                   -> adv   (the advection of the state, as k_rows_advect5 writes it)
//     dp = -(ddxw u + dxw du + ddyw v + dyw dv)               -> dadv  (its directional derivative along dw)
// One group per row pair, two rows per complex transform as in v5 / k_rows_vjp: eight c2r, two r2c.  Plane order
//     u, ddxw, dxw, du | v, ddyw, dyw, dv
// Each perturbation transform is folded into dp as soon as its state partner is there, and u (v) is dead once p has taken
// u dxw (v dyw): besides p and dp ONE kept transform (`k`) and the working one (`w`) are live -- four arrays of EPT elements, as
// in k_rows_vjp.  The eight inverse transforms are ONE piece of code in a loop that is not unrolled (the plane and what its
// transform is folded into are selected by the loop index): unrolled, the whole row pair is a single scheduling region in
// which the compiler keeps the loads, twiddles and addresses of several transforms in flight, and every instantiation with
// EPT >= 12 spilled in fp64.  Plain (non-split) plane layout, rows read right before use (no prefetch registers).
// PART = 0: both outputs in one sweep; 1: p only, 2: dp only (re-reading the state planes) -- the two-pass form for the sizes
// whose one-pass form would not fit the register file.
template <typename T, int N, int EPT, int THR, int PART>
__global__ __launch_bounds__((RowGeom<T, N, EPT, THR>::THREADS)) void k_rows_jvp(const cx<T>* __restrict__ planes,
                                                                                 const cx<T>* __restrict__ dplanes,
                                                                                 size_t plane_stride, cx<T>* __restrict__ adv,
                                                                                 cx<T>* __restrict__ dadv,
                                                                                 const cx<T>* __restrict__ tw, long npairs, int ld) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT, THR>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    constexpr bool DO_P = (PART != 2), DO_D = (PART != 1);
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    const long stride = (long)gridDim.x * Gm::GROUPS;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const long iters = (npairs + stride - 1) / stride;   // every group runs the same number of iterations (workgroup barriers)
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const size_t off = (size_t)cur * 2 * (size_t)ld;
        cx<T> k[EPT], w[EPT];
        [[maybe_unused]] cx<T> p[EPT], dp[EPT];
#pragma unroll
        for (int t = 0; t < EPT; ++t) {
            if constexpr (DO_P) p[t] = mk<T>((T)0, (T)0);
            if constexpr (DO_D) dp[t] = mk<T>((T)0, (T)0);
        }
        // s = 4 c + r: velocity component c (0: u with dx w, 1: v with dy w), role r of the transform
        //   r = 0: k <- u        r = 1: dp += d(dxw) k        r = 2: p += k dxw, k <- dxw        r = 3: dp += k du
#pragma unroll 1
        for (int s = 0; s < 8; s += (DO_D ? 1 : 2)) {   // (p alone: the state's planes only)
            const int c = s >> 2, r = s & 3;
            const int f = (r == 0 || r == 3) ? c : 2 + c;
            const cx<T>* rowA = ((r & 1) ? dplanes : planes) + (size_t)f * plane_stride + off;
            {
                RawPair<T, EPT> H;
                load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
                pack_herm<T, N, EPT, WG>(w, H, lds, j);
            }
            tile_fft<T, N, EPT, +1, 1, true, WG>(w, lds, tw, j, 0);
            if (r == 0) {
#pragma unroll
                for (int t = 0; t < EPT; ++t) k[t] = w[t];
            } else if (r == 2) {
#pragma unroll
                for (int t = 0; t < EPT; ++t) {
                    if constexpr (DO_P) p[t] = mk<T>(p[t].x + k[t].x * w[t].x, p[t].y + k[t].y * w[t].y);
                    if constexpr (DO_D) k[t] = w[t];
                }
            } else {
                if constexpr (DO_D) {
#pragma unroll
                    for (int t = 0; t < EPT; ++t) dp[t] = mk<T>(dp[t].x + w[t].x * k[t].x, dp[t].y + w[t].y * k[t].y);
                }
            }
        }
        if constexpr (DO_P) {
#pragma unroll
            for (int t = 0; t < EPT; ++t) p[t] = mk<T>(-p[t].x, -p[t].y);
            tile_fft<T, N, EPT, -1, 1, true, WG>(p, lds, tw, j, 0);
            unpack_store_pair<T, N, EPT>(p, lds, adv + off, adv + off + ld, j, valid);
        }
        if constexpr (DO_D) {
#pragma unroll
            for (int t = 0; t < EPT; ++t) dp[t] = mk<T>(-dp[t].x, -dp[t].y);
            tile_fft<T, N, EPT, -1, 1, true, WG>(dp, lds, tw, j, 0);
            unpack_store_pair<T, N, EPT>(dp, lds, dadv + off, dadv + off + ld, j, valid);
        }
    }
}

// ---- row pass of a BUNDLE of tangents: one state, K perturbations -------------------------------------------------------------
// k_rows_jvp carries one perturbation per state, so K perturbations of one trajectory transform the state's four planes K times.
// Here a group transforms them ONCE per row pair, keeps the four physical-space rows and folds the K perturbations against them:
//     p    = -(u dxw + v dyw)                                          -> adv            (skipped when adv is null)
//     dp_k = -(ddxw_k u + dxw du_k + ddyw_k v + dyw dv_k)              -> dadv + k dtan_stride,      k < ntan
// 4 + 4 K c2r and 1 + K r2c per row pair (K replicated k_rows_jvp sweeps: 8 K and 2 K).  The sums are accumulated in the order of
// k_rows_jvp, term by term; the BITS are still not the single-tangent kernel's: hipcc contracts multiply-adds kernel by kernel, and
// the two differ in the last place (measured: 2.5e-16 fp64, 1e-7 fp32 relative L2).  Member k does have the bits of the
// K = 1 bundle call, whatever the other members hold.
// THE STASH.  Every transform of a group leaves element j + t G of the row pair in register t of lane j, so the lane that needs
// u, dxw, v, dyw at an element is the lane that produced them: the kept rows are lane-private and need no barrier.  They live in
// LDS behind the groups' exchange buffers, 4 EPT elements per lane, stored [plane][t][thread of the workgroup]: consecutive lanes
// touch consecutive 8 / 16-byte slots whatever the group size, so every stash access is conflict free (a per-group layout puts the
// groups of one wave a multiple of the bank period apart).  Live registers: the working transform and ONE accumulator (p, then
// dp_k) -- two arrays of EPT elements against the four of k_rows_jvp, which is why the 12-element fp64 sizes need no second pass.
// LDS per lane is 5 EPT elements (exchange + stash): 640 B in fp64 at EPT = 8, so occupancy is set by LDS, not by registers
// (BundleGeom, bundle_two_pass below).  Workgroups are ONE wave (or one group where a group is wider): the LDS per lane is fixed,
// so smaller workgroups cost no occupancy and pack the CU's 160 KB in finer grains.
// The state's four transforms and the 4 K tangent transforms are two loops that are NOT unrolled, for k_rows_jvp's reason.
template <typename T, int N, int EPT>
struct BundleGeom {
    static constexpr int G = N / EPT;
    static constexpr int THREADS = G >= 64 ? G : 64;
    static constexpr int GROUPS = THREADS / G;
    static constexpr int XCH_PER_GROUP = lds_elems<N, EPT, 1, true>();
    static constexpr int STASH_ELEMS = 4 * EPT * THREADS;                 // == 4 N per group
    static constexpr size_t LDS_BYTES = ((size_t)GROUPS * XCH_PER_GROUP + STASH_ELEMS) * sizeof(cx<T>);
};

template <typename T, int N, int EPT>
__global__ __launch_bounds__((BundleGeom<T, N, EPT>::THREADS)) void k_rows_jvp_bundle(
    const cx<T>* __restrict__ planes, size_t plane_stride, const cx<T>* __restrict__ dplanes, size_t dplane_stride,
    size_t dtan_stride, cx<T>* __restrict__ adv, cx<T>* __restrict__ dadv, size_t dadv_stride, const cx<T>* __restrict__ tw,
    long npairs, int ld, int ntan) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = BundleGeom<T, N, EPT>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    constexpr int TH = Gm::THREADS;
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::XCH_PER_GROUP;
    cx<T>* stash = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)Gm::GROUPS * Gm::XCH_PER_GROUP + threadIdx.x;
    const long stride = (long)gridDim.x * Gm::GROUPS;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const long iters = (npairs + stride - 1) / stride;   // every group runs the same number of iterations (workgroup barriers)
    // blockIdx.y: the segment of the tangents this workgroup folds (see the launcher); segment 0 also writes p
    const int kper = (ntan + (int)gridDim.y - 1) / (int)gridDim.y;
    const int k_lo = (int)blockIdx.y * kper, k_hi = min(ntan, k_lo + kper);
    const bool do_p = adv && blockIdx.y == 0;   // block-uniform
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const size_t off = (size_t)cur * 2 * (size_t)ld;
        cx<T> w[EPT], a[EPT];
#pragma unroll
        for (int t = 0; t < EPT; ++t) a[t] = mk<T>((T)0, (T)0);
        // the state: stash slot s = 0 .. 3 holds u, dxw, v, dyw (planes 0, 2, 1, 3); p takes u dxw at s = 1 and v dyw at s = 3
#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
            const int f = (s & 1) ? 2 + (s >> 1) : (s >> 1);
            const cx<T>* rowA = planes + (size_t)f * plane_stride + off;
            {
                RawPair<T, EPT> H;
                load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
                pack_herm<T, N, EPT, WG>(w, H, lds, j);
            }
            tile_fft<T, N, EPT, +1, 1, true, WG>(w, lds, tw, j, 0);
#pragma unroll
            for (int t = 0; t < EPT; ++t) stash[(s * EPT + t) * TH] = w[t];
            if ((s & 1) && do_p) {
#pragma unroll
                for (int t = 0; t < EPT; ++t) {
                    const cx<T> k = stash[((s - 1) * EPT + t) * TH];
                    a[t] = mk<T>(a[t].x + k.x * w[t].x, a[t].y + k.y * w[t].y);
                }
            }
        }
        if (do_p) {
#pragma unroll
            for (int t = 0; t < EPT; ++t) a[t] = mk<T>(-a[t].x, -a[t].y);
            tile_fft<T, N, EPT, -1, 1, true, WG>(a, lds, tw, j, 0);
            unpack_store_pair<T, N, EPT>(a, lds, adv + off, adv + off + ld, j, valid);
        }
        // the tangents: transform q = 0 .. 3 of tangent k is d(dxw), du, d(dyw), dv (planes 2, 0, 3, 1), folded against stash slot q
#pragma unroll 1
        for (int kt = k_lo; kt < k_hi; ++kt) {
            const cx<T>* dset = dplanes + (size_t)kt * dtan_stride + off;
#pragma unroll
            for (int t = 0; t < EPT; ++t) a[t] = mk<T>((T)0, (T)0);
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                const int f = (q & 1) ? (q >> 1) : 2 + (q >> 1);
                const cx<T>* rowA = dset + (size_t)f * dplane_stride;
                {
                    RawPair<T, EPT> H;
                    load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
                    pack_herm<T, N, EPT, WG>(w, H, lds, j);
                }
                tile_fft<T, N, EPT, +1, 1, true, WG>(w, lds, tw, j, 0);
#pragma unroll
                for (int t = 0; t < EPT; ++t) {
                    const cx<T> k = stash[(q * EPT + t) * TH];
                    a[t] = mk<T>(a[t].x + w[t].x * k.x, a[t].y + w[t].y * k.y);
                }
            }
#pragma unroll
            for (int t = 0; t < EPT; ++t) a[t] = mk<T>(-a[t].x, -a[t].y);
            tile_fft<T, N, EPT, -1, 1, true, WG>(a, lds, tw, j, 0);
            cx<T>* o = dadv + (size_t)kt * dadv_stride + off;
            unpack_store_pair<T, N, EPT>(a, lds, o, o + ld, j, valid);
        }
    }
}

// ---- row pass of a BUNDLE of cotangents: one state, K cotangents (the reverse-mode counterpart of k_rows_jvp_bundle) ----------
// k_rows_vjp carries one cotangent per state, so K cotangents of one trajectory transform the state's four planes K times.  Here a
// group transforms them ONCE per row pair into the stash of k_rows_jvp_bundle (same geometry, same slots: u, dxw, v, dyw from
// planes 0, 2, 1, 3), then per cotangent k: one c2r of nbar_k, and four products  nbar_k x stash[s]  each followed by its r2c and
// store into that cotangent's OWN plane set -- out of place, the state's planes must survive for the next cotangent group:
//     Y0 = nbar dxw,  Y1 = nbar dyw,  Y2 = nbar u,  Y3 = nbar v             (k_rows_vjp's partner order)
//     plane f of cotangent k  ->  yout + f * yplane_stride + k * ytan_stride
// 4 + 5 K transforms per row pair instead of 9 K.  Live registers: nbar_k and the working array, two arrays of EPT elements.  The
// cotangent loop and the four-product loop are NOT unrolled, for k_rows_jvp's reason.  Every member runs the same code on its own
// data: member k has the bits of the K = 1 call whatever the other members hold, and whatever the cut of the cotangents into
// blockIdx.y segments (each segment redoes the state's transforms; see the launcher).  Against k_rows_vjp the fp32 bits were equal
// at every size tested and the fp64 bits differ in the last place (at most 4.0e-16 relative L2 of the four spectra, n = 8 .. 1536,
// tests/test_ns2d_cobundle_gpu.py): hipcc contracts the multiply-adds of the transforms kernel by kernel, as for k_rows_jvp_bundle.
template <typename T, int N, int EPT>
__global__ __launch_bounds__((BundleGeom<T, N, EPT>::THREADS)) void k_rows_vjp_bundle(
    const cx<T>* __restrict__ planes, size_t plane_stride, const cx<T>* __restrict__ nbar, size_t nbar_stride,
    cx<T>* __restrict__ yout, size_t yplane_stride, size_t ytan_stride, const cx<T>* __restrict__ tw, long npairs, int ld, int ncot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = BundleGeom<T, N, EPT>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    constexpr int TH = Gm::THREADS;
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::XCH_PER_GROUP;
    cx<T>* stash = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)Gm::GROUPS * Gm::XCH_PER_GROUP + threadIdx.x;
    const long stride = (long)gridDim.x * Gm::GROUPS;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const long iters = (npairs + stride - 1) / stride;   // every group runs the same number of iterations (workgroup barriers)
    const int kper = (ncot + (int)gridDim.y - 1) / (int)gridDim.y;
    const int k_lo = (int)blockIdx.y * kper, k_hi = min(ncot, k_lo + kper);
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const size_t off = (size_t)cur * 2 * (size_t)ld;
        cx<T> w[EPT], nb[EPT];
        // the state: stash slot s = 0 .. 3 holds u, dxw, v, dyw (planes 0, 2, 1, 3)
#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
            const int f = (s & 1) ? 2 + (s >> 1) : (s >> 1);
            const cx<T>* rowA = planes + (size_t)f * plane_stride + off;
            {
                RawPair<T, EPT> H;
                load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
                pack_herm<T, N, EPT, WG>(w, H, lds, j);
            }
            tile_fft<T, N, EPT, +1, 1, true, WG>(w, lds, tw, j, 0);
#pragma unroll
            for (int t = 0; t < EPT; ++t) stash[(s * EPT + t) * TH] = w[t];
        }
#pragma unroll 1
        for (int kt = k_lo; kt < k_hi; ++kt) {
            {
                const cx<T>* rowA = nbar + (size_t)kt * nbar_stride + off;
                RawPair<T, EPT> H;
                load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
                pack_herm<T, N, EPT, WG>(nb, H, lds, j);
            }
            tile_fft<T, N, EPT, +1, 1, true, WG>(nb, lds, tw, j, 0);
            cx<T>* yset = yout + (size_t)kt * ytan_stride + off;
            // stash slot s (u, dxw, v, dyw) is the partner of plane 2, 0, 3, 1
#pragma unroll 1
            for (int s = 0; s < 4; ++s) {
                const int f = (s & 1) ? (s >> 1) : 2 + (s >> 1);
#pragma unroll
                for (int t = 0; t < EPT; ++t) {
                    const cx<T> k = stash[(s * EPT + t) * TH];
                    w[t] = mk<T>(nb[t].x * k.x, nb[t].y * k.y);
                }
                tile_fft<T, N, EPT, -1, 1, true, WG>(w, lds, tw, j, 0);
                cx<T>* o = yset + (size_t)f * yplane_stride;
                unpack_store_pair<T, N, EPT>(w, lds, o, o + ld, j, valid);
            }
        }
    }
}

// The out-of-place form of k_rows_vjp for ONE cotangent: reads the state's planes and nbar (`gplane`), writes the four Y rows to
// yout + f * yout_stride instead of over the planes -- the row pass of the cotangent bundle at the sizes whose stash does not fit
// (bundle_two_pass), launched once per cotangent.  A kernel of its own: k_rows_vjp keeps its signature and its code.
template <typename T, int N, int EPT, int THR>
__global__ __launch_bounds__((RowGeom<T, N, EPT, THR>::THREADS)) void k_rows_vjp_oop(const cx<T>* __restrict__ planes,
                                                                                     size_t plane_stride,
                                                                                     const cx<T>* __restrict__ gplane,
                                                                                     cx<T>* __restrict__ yout, size_t yout_stride,
                                                                                     const cx<T>* __restrict__ tw, long npairs,
                                                                                     int ld) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT, THR>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    const long stride = (long)gridDim.x * Gm::GROUPS;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const long iters = (npairs + stride - 1) / stride;   // every group runs the same number of iterations (workgroup barriers)
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const size_t off = (size_t)cur * 2 * (size_t)ld;
        cx<T> nb[EPT], w[EPT];
        {
            RawPair<T, EPT> H;
            load_raw<T, N, EPT>(H, gplane + off, gplane + off + ld, j);
            pack_herm<T, N, EPT, WG>(nb, H, lds, j);
        }
        tile_fft<T, N, EPT, +1, 1, true, WG>(nb, lds, tw, j, 0);
        // partner plane s of output plane f: dxw, dyw, u, v (planes 2, 3, 0, 1)
#pragma unroll 1
        for (int f = 0; f < 4; ++f) {
            const cx<T>* rowA = planes + (size_t)(f ^ 2) * plane_stride + off;
            {
                RawPair<T, EPT> H;
                load_raw<T, N, EPT>(H, rowA, rowA + ld, j);
                pack_herm<T, N, EPT, WG>(w, H, lds, j);
            }
            tile_fft<T, N, EPT, +1, 1, true, WG>(w, lds, tw, j, 0);
#pragma unroll
            for (int t = 0; t < EPT; ++t) w[t] = mk<T>(nb[t].x * w[t].x, nb[t].y * w[t].y);
            tile_fft<T, N, EPT, -1, 1, true, WG>(w, lds, tw, j, 0);
            cx<T>* o = yout + (size_t)f * yout_stride + off;
            unpack_store_pair<T, N, EPT>(w, lds, o, o + ld, j, valid);
        }
    }
}

// ---- row pass, one plane per transform ("v5") --------------------------------------------------
// Round 1 rode two PLANES of one row through a complex transform, so the transformed velocity rows of BOTH rows of a pair
// stayed live while the gradient planes were transformed (256 VGPR + 84 AGPR, one wave per SIMD at 1024^2 fp64; kernels v3 / v4,
// removed in round 5 with the LDS-DMA staged v6 -- docs/history/DESIGN_rounds_1-4.md section 4).  Here the two ROWS of a pair ride
// through one transform of ONE plane:  Z = P(row a) + i P(row b)  ->  real part = field on row a, imaginary part = field on row b, and
//     p.x = -(vx_a dxw_a + vy_a dyw_a),  p.y = -(vx_b dxw_b + vy_b dyw_b)
// accumulates plane by plane (order u^, dx w^, v^, dy w^): one kept transform + the working one + the product +
// the next plane's half rows in flight -- half the live state, same loads / stores / transform count.
// SP = 0: rows (2p, 2p+1).  SP = 1 (split column plans): rows (r, r + N/2).  The planes then hold, for every field, the
// N/2-point column transforms of the even spectral rows (E, workspace rows [0, N/2)) and of the odd ones (O, rows [N/2, N)); the
// column transform is completed here,  a = E + w O,  b = E - w O,  w = exp(+2 pi i r / N), and the advection spectra A_r, A_{r+N/2}
// leave folded as S = A_r + A_{r+N/2},  D = (A_r - A_{r+N/2}) exp(-2 pi i r / N), which the two parity workgroups of the column
// pass transform with N/2 points each.
template <typename T, int N, int EPT, int THR, int SP, int MINW, int PF = 1, int NYQ = 0>
__global__ __launch_bounds__((RowGeom<T, N, EPT, THR>::THREADS), MINW) void k_rows_advect5(
    const cx<T>* __restrict__ planes, size_t plane_stride, cx<T>* __restrict__ adv, const cx<T>* __restrict__ tw,
    long npairs, int ld, int kc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT, THR>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    constexpr int N2 = N / 2;
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    const long stride = (long)gridDim.x * Gm::GROUPS;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const long iters = (npairs + stride - 1) / stride;
    // first row of pair p; the second row sits `second` elements further
    auto row_a = [&](long p) -> size_t {
        return SP ? (size_t)((p / N2) * N + (p % N2)) * (size_t)ld : (size_t)p * 2 * (size_t)ld;
    };
    const size_t second = SP ? (size_t)N2 * ld : (size_t)ld;

    // PF = 1: half rows (a, b) -- or (E, O) -- of the plane whose turn is NEXT, in flight during the current transform;
    // PF = 0: loaded right before use (fewer live registers: occupancy hides the latency instead)
    RawPair<T, EPT> H;
    if constexpr (PF) {
        const size_t off = row_a(pair < npairs ? pair : npairs - 1);
        load_raw<T, N, EPT, NYQ>(H, planes + off, planes + off + second, j);
    }
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const long nxt = (pair + stride < npairs) ? pair + stride : npairs - 1;
        const size_t off = row_a(cur), offn = row_a(nxt);
        cx<T> wf = mk<T>((T)1, (T)0), wi = wf;
        if constexpr (SP) {
            wf = tw[(int)(cur % N2)];   // exp(-2 pi i r / N)
            wi = cconj(wf);
        }
        cx<T> za[EPT], x[EPT], p[EPT];
        // H -> Hermitian-packed sequence -> transform; the next plane's loads are issued in between
        auto field = [&](cx<T>(&out)[EPT], const cx<T>* thisA, const cx<T>* nextA) {
            if constexpr (!PF) load_raw<T, N, EPT, NYQ>(H, thisA, thisA + second, j);
            if constexpr (SP) {
#pragma unroll
                for (int t = 0; t < EPT / 2; ++t) {
                    const cx<T> o = cmul(H.b[t], wi);
                    H.b[t] = H.a[t] - o;
                    H.a[t] = H.a[t] + o;
                }
                if constexpr (!NYQ) {
                    const cx<T> o = cmul(H.bn, wi);
                    H.bn = H.an - o;
                    H.an = H.an + o;
                }
            }
            pack_herm<T, N, EPT, WG, NYQ>(out, H, lds, j);
            if constexpr (PF) load_raw<T, N, EPT, NYQ>(H, nextA, nextA + second, j);
            tile_fft<T, N, EPT, +1, 1, true, WG>(out, lds, tw, j, 0);
        };
        const cx<T>* P0 = planes + off;
        const cx<T>* P1 = planes + plane_stride + off;
        const cx<T>* P2 = planes + 2 * plane_stride + off;
        const cx<T>* P3 = planes + 3 * plane_stride + off;
        field(za, P0, P2);   // vx   (next: dx w)
        field(x, P2, P1);    // dx w (next: v^)
#pragma unroll
        for (int t = 0; t < EPT; ++t) p[t] = mk<T>(za[t].x * x[t].x, za[t].y * x[t].y);
        field(za, P1, P3);               // vy   (next: dy w)
        field(x, P3, planes + offn);     // dy w (next: u^ of the next pair)
#pragma unroll
        for (int t = 0; t < EPT; ++t) p[t] = mk<T>(-(p[t].x + za[t].x * x[t].x), -(p[t].y + za[t].y * x[t].y));

        const int jf = j;
        tile_fft<T, N, EPT, -1, 1, true, WG>(p, lds, tw, jf, 0);
        if constexpr (SP) {
            // unpack the two real-row spectra and fold them for the parity workgroups of the column pass
#pragma unroll
            for (int t = 0; t < EPT; ++t) lds[lds_addr<EPT, 1, true>(jf + t * G, 0)] = p[t];
            group_sync<WG>();
            const T half = (T)0.5;
            cx<T>* outS = adv + off;
            cx<T>* outD = adv + off + second;
#pragma unroll
            for (int t = 0; t < EPT / 2; ++t) {
                const int k = jf + t * G;
                const cx<T> A = p[t];
                const cx<T> Bm = lds[lds_addr<EPT, 1, true>((N - k) % N, 0)];
                const cx<T> X0 = mk<T>((A.x + Bm.x) * half, (A.y - Bm.y) * half);   // spectrum of row r
                const cx<T> X1 = mk<T>((A.y + Bm.y) * half, (Bm.x - A.x) * half);   // spectrum of row r + N/2
                if (valid && k < kc) {
                    outS[k] = X0 + X1;
                    outD[k] = cmul(X0 - X1, wf);
                }
            }
            if (jf == 0 && valid && N / 2 < kc) {
                const cx<T> A = p[EPT / 2];
                const cx<T> X0 = mk<T>(A.x, (T)0), X1 = mk<T>(A.y, (T)0);
                outS[N / 2] = X0 + X1;
                outD[N / 2] = cmul(X0 - X1, wf);
            }
            group_sync<WG>();
        } else {
            unpack_store_pair<T, N, EPT>(p, lds, adv + off, adv + off + second, jf, valid, kc);
        }
    }
}

// ---- row pass, cross-lane transforms ("v7", 1024 points on two-wave groups) ------------------------------------
// v5 with the three-exchange Stockham transform replaced by xl_fft1024 (tcfd_fft.hpp): one LDS exchange per
// transform, the other two are register <-> lane bit transpositions inside a wave (v_permlane32/16_swap, DPP).
// The four inverse transforms leave the physical rows in the fixed permutation `pi`; the point-wise product does
// not care, and the forward transform of the product starts from `pi` and ends in natural order.
// LDS stores per row pair: 18 -> 8 exchange-equivalents of 16 KB; workgroup barriers per pair: ~40 -> ~20.
template <typename T, int THR, int SP, int MINW, int PF, int NYQ = 0>
__global__ __launch_bounds__(128, MINW) void k_rows_advect7(
    const cx<T>* __restrict__ planes, size_t plane_stride, cx<T>* __restrict__ adv, const cx<T>* __restrict__ tw,
    long npairs, int ld, int kc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int N = 1024, EPT = 8, G = 128, N2 = N / 2;
    constexpr bool WG = true;
    constexpr bool SWZ7 = false;     // mirror accesses without the Stockham swizzle: no bank conflicts (see pack_herm)
    const int j = threadIdx.x;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw);
    const long stride = (long)gridDim.x;
    long pair = (long)blockIdx.x;
    const long iters = (npairs + stride - 1) / stride;
    auto row_a = [&](long p) -> size_t {
        return SP ? (size_t)((p / N2) * N + (p % N2)) * (size_t)ld : (size_t)p * 2 * (size_t)ld;
    };
    const size_t second = SP ? (size_t)N2 * ld : (size_t)ld;
    const XlTw<T> xtw = xl_load_tw<T>(tw, j);
    NoHook nohook;

    RawPair<T, EPT> H;
    if constexpr (PF) {
        const size_t off = row_a(pair < npairs ? pair : npairs - 1);
        load_raw<T, N, EPT, NYQ>(H, planes + off, planes + off + second, j);
    }
    for (long it = 0; it < iters; ++it, pair += stride) {
        const bool valid = pair < npairs;
        const long cur = valid ? pair : npairs - 1;
        const long nxt = (pair + stride < npairs) ? pair + stride : npairs - 1;
        const size_t off = row_a(cur), offn = row_a(nxt);
        cx<T> wf = mk<T>((T)1, (T)0), wi = wf;
        if constexpr (SP) {
            wf = tw[(int)(cur % N2)];   // exp(-2 pi i r / N)
            wi = cconj(wf);
        }
        cx<T> za[EPT], x[EPT], p[EPT];
        auto field = [&](cx<T>(&out)[EPT], const cx<T>* thisA, const cx<T>* nextA) {
            if constexpr (!PF) load_raw<T, N, EPT, NYQ>(H, thisA, thisA + second, j);
            if constexpr (SP) {
#pragma unroll
                for (int t = 0; t < EPT / 2; ++t) {
                    const cx<T> o = cmul(H.b[t], wi);
                    H.b[t] = H.a[t] - o;
                    H.a[t] = H.a[t] + o;
                }
                if constexpr (!NYQ) {
                    const cx<T> o = cmul(H.bn, wi);
                    H.bn = H.an - o;
                    H.an = H.an + o;
                }
            }
            pack_herm<T, N, EPT, WG, NYQ, SWZ7>(out, H, lds, j);
            if constexpr (PF) load_raw<T, N, EPT, NYQ>(H, nextA, nextA + second, j);
            xl_fft1024<T, +1, 1>(out, lds, xtw, j, nohook);
        };
        const cx<T>* P0 = planes + off;
        const cx<T>* P1 = planes + plane_stride + off;
        const cx<T>* P2 = planes + 2 * plane_stride + off;
        const cx<T>* P3 = planes + 3 * plane_stride + off;
        field(za, P0, P2);   // vx   (next: dx w)
        field(x, P2, P1);    // dx w (next: v^)
#pragma unroll
        for (int t = 0; t < EPT; ++t) p[t] = mk<T>(za[t].x * x[t].x, za[t].y * x[t].y);
        field(za, P1, P3);               // vy   (next: dy w)
        field(x, P3, planes + offn);     // dy w (next: u^ of the next pair)
#pragma unroll
        for (int t = 0; t < EPT; ++t) p[t] = mk<T>(-(p[t].x + za[t].x * x[t].x), -(p[t].y + za[t].y * x[t].y));

        xl_fft1024<T, -1, 1>(p, lds, xtw, j, nohook);   // pi -> natural order
        // unpack the two real-row spectra (mirror through the exchange buffer)
        const cx<T>* mir = lds + lds_addr<EPT, 1, SWZ7>(N - j, 0);
#pragma unroll
        for (int t = 0; t < EPT; ++t) lds[lds_addr<EPT, 1, SWZ7>(j + t * G, 0)] = p[t];
        group_sync<WG>();
        const T half = (T)0.5;
        cx<T>* out0 = adv + off;
        cx<T>* out1 = adv + off + second;
#pragma unroll
        for (int t = 0; t < EPT / 2; ++t) {
            const int k = j + t * G;
            const cx<T> A = p[t];
            const cx<T> Bm = (j == 0 && t == 0) ? p[0] : mir[-t * G];   // element N - k; k = 0 mirrors itself
            const cx<T> X0 = mk<T>((A.x + Bm.x) * half, (A.y - Bm.y) * half);   // spectrum of the first row
            const cx<T> X1 = mk<T>((A.y + Bm.y) * half, (Bm.x - A.x) * half);   // spectrum of the second row
            if (valid && k < kc) {
                if constexpr (SP) {   // folded for the parity workgroups of the column pass
                    out0[k] = X0 + X1;
                    out1[k] = cmul(X0 - X1, wf);
                } else {
                    out0[k] = X0;
                    out1[k] = X1;
                }
            }
        }
        if (j == 0 && valid && N2 < kc) {
            const cx<T> A = p[EPT / 2];
            const cx<T> X0 = mk<T>(A.x, (T)0), X1 = mk<T>(A.y, (T)0);
            if constexpr (SP) {
                out0[N2] = X0 + X1;
                out1[N2] = cmul(X0 - X1, wf);
            } else {
                out0[N2] = X0;
                out1[N2] = X1;
            }
        }
        group_sync<WG>();
    }
}

// real (rows, N) -> half spectrum (rows, m): first half of rfft2
template <typename T, int N, int EPT>
__global__ __launch_bounds__((RowGeom<T, N, EPT>::THREADS)) void k_rows_r2c(const T* __restrict__ in,
                                                                             cx<T>* __restrict__ out,
                                                                             const cx<T>* __restrict__ tw, long npairs,
                                                                             int m /* pitch of out */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const bool valid = pair < npairs;
    if (!valid) pair = npairs - 1;
    const size_t row0 = (size_t)pair * 2;
    cx<T> p[EPT];
#pragma unroll
    for (int t = 0; t < EPT; ++t) {
        const int e = j + t * G;
        p[t] = mk<T>(in[row0 * N + e], in[(row0 + 1) * N + e]);
    }
    tile_fft<T, N, EPT, -1, 1, true, WG>(p, lds, tw, j, 0);
    unpack_store_pair<T, N, EPT>(p, lds, out + row0 * (size_t)m, out + (row0 + 1) * (size_t)m, j, valid);
}

// half spectrum (rows, m) -> real (rows, N): second half of irfft2 (scale applied by the column pass)
template <typename T, int N, int EPT>
__global__ __launch_bounds__((RowGeom<T, N, EPT>::THREADS)) void k_rows_c2r(const cx<T>* __restrict__ in,
                                                                             T* __restrict__ out,
                                                                             const cx<T>* __restrict__ tw, long npairs,
                                                                             int m /* pitch of in */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    long pair = (long)blockIdx.x * Gm::GROUPS + grp;
    const bool valid = pair < npairs;
    if (!valid) pair = npairs - 1;
    const size_t row0 = (size_t)pair * 2;
    cx<T> z[EPT];
    load_herm_pair<T, N, EPT>(z, in + row0 * (size_t)m, in + (row0 + 1) * (size_t)m, j);
    tile_fft<T, N, EPT, +1, 1, true, WG>(z, lds, tw, j, 0);
    if (valid) {
#pragma unroll
        for (int t = 0; t < EPT; ++t) {
            const int e = j + t * G;
            out[row0 * N + e] = z[t].x;
            out[(row0 + 1) * N + e] = z[t].y;
        }
    }
}

// Second half of irfft2 + the data-generation drivers' bilinear subsample in ONE pass (fno/data_gen/data_gen_McWilliams2d.py:
// 158-163: irfft2 -> F.interpolate(size = (N / S, N / S), mode = "bilinear")).  For an even integer factor S the sample point
// of output pixel (r, c) is (S r + (S - 1) / 2, S c + (S - 1) / 2): exactly between rows S r + S / 2 - 1 and S r + S / 2 and
// between the two columns of the same numbers, every weight 1 / 2.  A group transforms those two rows as ONE complex sequence
// (any two rows pack, they need not be neighbours in the pair index) -- so the rows the subsample never looks at are not
// transformed at all --, the horizontal neighbour is one lane away (element j + t G of lane j: S <= G keeps both in a wave),
// the vertical one is the other component of the same register.  Arithmetic in ATen's order, 0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c +
// 0.5 d) with a, b on the upper row: at S = 2 (same row pairs as k_rows_c2r) the result is bit-identical to irfft2 followed by
// F.interpolate, beyond it agrees to rounding (which two rows share a transform shows in the last bit); the full-size field
// -- written and read again by the two-step path, 2.25 x the bytes of this one at S = 2 -- never exists.
template <typename T, int N, int EPT>
__global__ __launch_bounds__((RowGeom<T, N, EPT>::THREADS)) void k_rows_c2r_sub(const cx<T>* __restrict__ in,
                                                                                 T* __restrict__ out,
                                                                                 const cx<T>* __restrict__ tw, long nrows,
                                                                                 int m /* pitch of in */, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using Gm = RowGeom<T, N, EPT>;
    constexpr int G = Gm::G;
    constexpr bool WG = (G > 64);
    const int grp = threadIdx.x / G;
    const int j = threadIdx.x % G;
    cx<T>* lds = reinterpret_cast<cx<T>*>(smem_raw) + (size_t)grp * Gm::LDS_PER_GROUP;
    long orow = (long)blockIdx.x * Gm::GROUPS + grp;          // output row over all fields
    const bool valid = orow < nrows;
    if (!valid) orow = nrows - 1;
    const int NS = N / S;
    const long f = orow / NS;
    const int r = (int)(orow - f * NS);
    const size_t row0 = (size_t)f * N + (size_t)r * S + (S / 2 - 1);
    cx<T> z[EPT];
    load_herm_pair<T, N, EPT>(z, in + row0 * (size_t)m, in + (row0 + 1) * (size_t)m, j);
    tile_fft<T, N, EPT, +1, 1, true, WG>(z, lds, tw, j, 0);
    T* orow_p = out + (size_t)orow * NS;
#pragma unroll
    for (int t = 0; t < EPT; ++t) asm volatile("" : "+v"(z[t].x), "+v"(z[t].y));   // the transform ends here: nothing below
                                                                                  // may be contracted into its last stage
#pragma unroll
    for (int t = 0; t < EPT; ++t) {
        const int e = j + t * G;
        const T bx = __shfl_down(z[t].x, 1), by = __shfl_down(z[t].y, 1);
        if (valid && (e & (S - 1)) == S / 2 - 1) {
            const T up = (T)0.5 * z[t].x + (T)0.5 * bx, lo = (T)0.5 * z[t].y + (T)0.5 * by;
            orow_p[e / S] = (T)0.5 * up + (T)0.5 * lo;
        }
    }
}

// ------------------------------------------------------------------ launch helpers
// Dynamic LDS above 64 KB needs a function attribute, and the attribute belongs to the function instance of ONE device:
// it is set once per (kernel, device), tracked by a bit mask at the launch site (one process may drive several GPUs
// from several host threads).
struct DevOnce { std::atomic<unsigned long long> mask{0}; };
template <typename K>
static int set_lds(DevOnce& once, K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (once.mask.load(std::memory_order_acquire) & bit) return 0;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)bytes));
    once.mask.fetch_or(bit, std::memory_order_release);
    return 0;
}

// tiles of C columns narrower than a 128-byte line: how many of them share a line (0: whole lines, nothing to group).
// TCFD_PAIR_XCD = 0 switches the XCD grouping off, 2 limits it to pairs (the round-1 form).
template <typename T, int C>
static int line_group(const tcfd_ns2d_plan* p) {
    constexpr int bytes = C * (int)sizeof(cx<T>);
    if (bytes >= 128 || p->tune.pair_xcd == 0) return 0;
    // 16-byte tiles (the whole-column tiles of n = 4096, no other size has them): all eight of a line; TCFD_PAIR_XCD = 4 keeps four
    // TCFD_PAIR_XCD = 8 groups eight tiles of ANY narrow width (two lines of 32-byte tiles): the same block -> tile map, reachable at
    // the small sizes where a test of its indexing costs milliseconds
    if (p->tune.pair_xcd == 8) return 8;
    const int lg = 128 / bytes > 4 ? ((bytes == 16 && p->tune.pair_xcd != 4) ? 8 : 4) : 128 / bytes;
    return p->tune.pair_xcd == 2 ? 2 : lg;
}

// {nu, drag, forcing_scale, l00} of field `b0` of the caller's batch on an ensemble plan (a chunk or a half batch starts there), else null
template <typename T>
static const T* ens_at(const tcfd_ns2d_plan* p, long b0) {
    return p->ens ? (const T*)p->ens + 4 * (size_t)b0 : nullptr;
}

template <typename T, int N, int MODE, int EPT, int C, int MINW = 1, int SP = 0>
static int launch_cols_v(const tcfd_ns2d_plan* p, ColArgs<T> a, long batch, hipStream_t st, bool no_forcing = false) {
    constexpr int NT = N >> SP;
    constexpr int G = NT / EPT;
    // + TCFD_COLS_LDS_PAD bytes: an experiment knob that caps the workgroups a CU takes (occupancy A/B without a rebuild)
    size_t lds = col_lds_bytes<T, NT, EPT, C>(false) + (size_t)p->tune.cols_lds_pad;
    a.m = p->m;
    a.ldw = p->ldw;
    a.ntiles = (p->m + C - 1) / C;
    if (a.nyq) a.ntiles = (p->m - 1) / C;   // packed Nyquist column: no lone tile (the caller checked the plan allows it)
    a.batch = (int)batch;
    a.kx = (const T*)p->kx;
    a.ky = (const T*)p->ky;
    a.lin = (const T*)p->lin;
    a.mask = (const T*)p->mask;
    a.forcing = (const cx<T>*)p->forcing;
    a.mask_r = (const T*)p->mask_r;
    a.mask_c = (const T*)p->mask_c;
    a.lin_r = (const T*)p->lin_r;
    a.lin_c = (const T*)p->lin_c;
    a.f_ptr = p->f_sparse ? (const int*)p->f_ptr : nullptr;
    a.f_col = (const int*)p->f_col;
    a.f_nnz = (p->f_sparse && p->f_nnz <= 32) ? p->f_nnz : 0;
    a.f_row = (const int*)p->f_row;
    a.f_val = (const cx<T>*)p->f_val;
    if (no_forcing) {   // the tangent of F carries no forcing term: this launch's copy of the arguments points at none
        a.forcing = nullptr;
        a.f_ptr = nullptr;
        a.f_nnz = 0;
    }
    a.sep = p->sep;
    a.lsep = p->sep;
    constexpr bool ENS_MODE = (MODE == MODE_CA || MODE == MODE_C || MODE == MODE_F || MODE == MODE_RES);
    if (!ENS_MODE) a.ens = nullptr;   // the other passes read neither L nor the forcing
    if (a.ens) {   // per-sample physics: the kernels form L from the laplacian's tables (tcfd_ns2d_plan_set_ensemble)
        a.lin = (const T*)p->lap;
        a.lin_r = (const T*)p->lap_r;
        a.lin_c = (const T*)p->lap_c;
        a.lsep = p->ens_sep;
    }
    a.keep_cols = p->keep_cols;
    a.tw = (const cx<T>*)(SP ? p->tw2 : p->tw);
    a.pair_xcd = line_group<T, C>(p);
    a.ablate = p->tune.ablate;
    a.nt_out = (MODE == MODE_C && p->tune.nt_out && a.u_out_ld == p->m) ? 1 : 0;   // (the caller's array: pitch m, not ldw)
    long blocks = batch * a.ntiles;
    if (a.pair_xcd) blocks = ((((long)(a.ntiles + a.pair_xcd - 1) / a.pair_xcd) * batch + 7) / 8) * 8 * a.pair_xcd;
    if (!a.h_out) a.h_out = a.h;
    const dim3 grid((unsigned)(blocks * (SP ? 2 : 1))), block(C * G);
    const int kind = MODE == MODE_A ? 0 : MODE == MODE_CA ? 2 : MODE == MODE_C ? 3 : 5;
    auto launch = [&](auto kern, DevOnce& once) -> int {
        if (int rc_ = set_lds(once, kern, lds)) return rc_;
        ProfScope prof(p, kind, st);
        hipLaunchKernelGGL(kern, grid, block, lds, st, a);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    // the packed Nyquist column needs tiles of two columns or more (emit_planes: S0 and SZ are NT elements each of the exchange buffer)
    constexpr bool NYQ_MODE = (MODE == MODE_A || MODE == MODE_CA || MODE == MODE_C) && C >= 2;
    if (a.nyq && !NYQ_MODE) return fail(TCFD_EINVAL, "packed Nyquist column on a column pass that cannot carry it");
    // 512-point tiles of 8 columns (1024^2 split plans and 512^2, fp64): cross-lane transforms unless TCFD_COLS_XL=0
    constexpr bool XL_OK = (NT == 512 && EPT == 8 && C == 8 && MODE != MODE_FWD && MODE != MODE_INV);
    if constexpr (XL_OK) {
        if (p->tune.cols_xl) {
            lds = col_lds_bytes<T, NT, EPT, C>(xl_col_direct<T>()) + (size_t)p->tune.cols_lds_pad;   // + the stage-two roots
            a.nt_planes = p->tune.nt_planes > 0;
            static DevOnce once_x, once_xn;
            if constexpr (ENS_MODE) {   // per-sample physics: the ENS instantiations
                static DevOnce once_xe, once_xne;
                if constexpr (NYQ_MODE) {
                    if (a.ens && a.nyq) return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 1, 1, 1>, once_xne);
                }
                if (a.ens) return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 1, 0, 1>, once_xe);
            }
            if constexpr (NYQ_MODE) {
                if (a.nyq) return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 1, 1>, once_xn);
            }
            return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 1, 0>, once_x);
        }
    }
    // 4-column tiles = the small, cache-resident problems: a whole pass's output would sit dirty in the L2s until the
    // end-of-kernel write-back; streamed out while the kernel still computes, 256^2 x 16 fp32 steps 4.6 % faster
    // (at 1024^2 the same hint costs 1-3 %)
    a.nt_planes = p->tune.nt_planes >= 0 ? p->tune.nt_planes : (C == 4 && EPT == 4);
    static DevOnce once, once_n;
    if constexpr (ENS_MODE) {
        static DevOnce once_e, once_ne;
        if constexpr (NYQ_MODE) {
            if (a.ens && a.nyq) return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 0, 1, 1>, once_ne);
        }
        if (a.ens) return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 0, 0, 1>, once_e);
    }
    if constexpr (NYQ_MODE) {
        if (a.nyq) return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 0, 1>, once_n);
    }
    return launch(k_cols<T, N, EPT, C, MODE, MINW, SP, 0, 0>, once);
}

#ifndef TCFD_SPLIT_A_MINW4
#define TCFD_SPLIT_A_MINW4 1
#endif
// Split plans: the column transform is cut radix-2 across the row pass so that a column tile is half as big
// and two workgroups share a CU.  Default: n = 1024 (fp64: the full tile would fill the CU's LDS; fp32: the half
// tiles are 16 columns = full 128-byte lines instead of 8).
template <typename T, int N>
static bool use_split(const tcfd_ns2d_plan* p) {
    const int force = p->tune.split;
    if (N < 16 || !is_pow2c(N)) return false;   // n = 3 * 2^k / 5 * 2^k: whole-column tiles only (split measured slower at 768: 160 vs 181 steps/s)
    if (force >= 0) return force != 0;
    // 4096: whole-column tiles are one (fp64) / two (fp32) columns wide -- 16 bytes of every row -- and fill the LDS with one
    // workgroup per CU; the 2048-point halves are the tiles of n = 2048 (2 / 8 columns)
    return N == 1024 || N == 4096;   // (768: split 160 vs plain 181 steps/s at one round of workgroups per launch)   // fp64: 7.99 vs 8.6 ms/step; fp32 (16-column, 128-byte tiles of 512 rows): 5.61 vs 6.05 ms/step
}

template <typename T, int N, int MODE>
static int launch_cols_split(const tcfd_ns2d_plan* p, ColArgs<T> a, long batch, hipStream_t st) {
    constexpr int H = N >= 16 ? N / 2 : 8;
    constexpr int EPT = Cfg<T, H>::COL_EPT, C = Cfg<T, H>::COLS;
    // 128 VGPRs per lane = two 512-lane workgroups per CU for the half-size fp64 tiles
    constexpr int MINW = (C * (H / EPT) == 512 && (MODE != MODE_A || TCFD_SPLIT_A_MINW4)) ? 4 : 1;
    if constexpr (N == 1024 && sizeof(T) == 4 && (MODE == MODE_A || MODE == MODE_CA)) {   // (see launch_cols: the same at 1024^2 x 64: CA 1.86 -> 1.74 ms)
        if (p->tune.f32_cols8) return launch_cols_v<T, N, MODE, 8, 8, 4, 1>(p, a, batch, st);
    }
    if constexpr (N >= 16 && MODE != MODE_FWD && MODE != MODE_INV)
        return launch_cols_v<T, N, MODE, EPT, C, MINW, 1>(p, a, batch, st);
    else
        return fail(TCFD_EINVAL, "split launch of an unsupported mode");
}

template <typename T, int N, int MODE>
static int launch_cols(const tcfd_ns2d_plan* p, ColArgs<T> a, long batch, hipStream_t st) {
    if constexpr (!is_pow2c(N)) {   // n = 3 * 2^k / 5 * 2^k: whole-column Stockham tiles (no split / cross-lane / packed-Nyquist variants)
        return launch_cols_v<T, N, MODE, Cfg<T, N>::COL_EPT, Cfg<T, N>::COLS>(p, a, batch, st);
    } else
    if constexpr (MODE != MODE_FWD && MODE != MODE_INV) {
        if (use_split<T, N>(p)) return launch_cols_split<T, N, MODE>(p, a, batch, st);
    }
    // small problems (few column tiles for 256 CUs, working set cache resident): narrow 4-column tiles and
    // 4 elements per lane give ~4x more, shorter workgroups (measured at 256^2 x 16 fp32: CA 29 -> 21 us)
    if constexpr ((N == 128 || N == 256) && (MODE == MODE_A || MODE == MODE_CA || MODE == MODE_C)) {
        const int force = p->tune.small_tiles;
        const long tiles = batch * ((p->m + Cfg<T, N>::COLS - 1) / Cfg<T, N>::COLS);
        if (force == 1 || (force != 0 && tiles < 2 * 256)) return launch_cols_v<T, N, MODE, 4, 4>(p, a, batch, st);
    }
    // 512-point fp64 tiles are 64 KB: capping the update kernels at 128 VGPRs lets TWO workgroups share a CU,
    // so one tile's memory phases overlap the other's transforms (measured at 512^2 x 256: CA 1.05 -> 0.87 ms)
    if constexpr (N == 512 && sizeof(T) == 8 && (MODE == MODE_CA || MODE == MODE_C)) {
        if (p->tune.two_wg) return launch_cols_v<T, N, MODE, 8, 8, 4>(p, a, batch, st);
    }
    // fp32 512-point tiles: 8 columns on the cross-lane transforms (one LDS exchange instead of two, 512-thread workgroups: two
    // per CU) for the passes that emit planes; the update-only pass keeps the 16-column Stockham tiles (measured per step at
    // 512^2 x 64: CA 0.453 -> 0.411 ms, C 0.086 -> 0.094, profiles/r06_f32_variants.txt).  TCFD_F32_COLS8=0: 16 columns everywhere
    if constexpr (N == 512 && sizeof(T) == 4 && (MODE == MODE_A || MODE == MODE_CA)) {
        if (p->tune.f32_cols8) return launch_cols_v<T, N, MODE, 8, 8, 4>(p, a, batch, st);
    }
    return launch_cols_v<T, N, MODE, Cfg<T, N>::COL_EPT, Cfg<T, N>::COLS>(p, a, batch, st);
}

// persistent row-pass grid: `per_cu` workgroups per CU, grid-stride over the row pairs
static long rows_grid(const tcfd_ns2d_plan* p, long want, int dflt_per_cu) {
    const int per_cu = p->tune.rows_blocks_per_cu > 0 ? p->tune.rows_blocks_per_cu : dflt_per_cu;
    return std::min<long>(want, 256L * per_cu);
}

template <typename T, int N, int EPT, int THR, int SP, int MINW, int PF = 1, int NYQ = 0>
static int launch_rows_advect5(const tcfd_ns2d_plan* p, const cx<T>* planes, size_t plane_stride, cx<T>* adv,
                               long batch, hipStream_t st, int nyq = 0) {
    if constexpr (!NYQ) {
        if (nyq) return launch_rows_advect5<T, N, EPT, THR, SP, MINW, PF, 1>(p, planes, plane_stride, adv, batch, st, 0);
    }
    using Gm = RowGeom<T, N, EPT, THR>;
    auto kern = k_rows_advect5<T, N, EPT, THR, SP, MINW, PF, NYQ>;
    static DevOnce lds_once;
    if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
    const long npairs = batch * (N / 2);
    // resident workgroups per CU: MINW waves per SIMD x 4 SIMDs / waves per workgroup (LDS allows it for every size)
    constexpr int WAVES = (Gm::THREADS + 63) / 64;
    constexpr int PER_CU = (4 * MINW / WAVES) > 0 ? (4 * MINW / WAVES) : 1;
    const long blocks = rows_grid(p, (npairs + Gm::GROUPS - 1) / Gm::GROUPS, PER_CU);
    ProfScope prof(p, 1, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, planes, plane_stride, adv,
                       (const cx<T>*)p->tw, npairs, p->ldw, p->keep_cols > 0 ? p->keep_cols : N);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T, int SP, int MINW, int PF, int NYQ = 0>
static int launch_rows_advect7(const tcfd_ns2d_plan* p, const cx<T>* planes, size_t plane_stride, cx<T>* adv,
                               long batch, hipStream_t st, int nyq = 0) {
    if constexpr (!NYQ) {
        if (nyq) return launch_rows_advect7<T, SP, MINW, PF, 1>(p, planes, plane_stride, adv, batch, st, 0);
    }
    auto kern = k_rows_advect7<T, 128, SP, MINW, PF, NYQ>;
    constexpr size_t lds = (size_t)(1024 + 1) * sizeof(cx<T>);   // + 1: the unpack reads slot N for lane 0 (value unused)
    const long npairs = batch * 512;
    const long blocks = rows_grid(p, npairs, 2 * MINW);   // two-wave workgroups: 2 per SIMD pair and wave slot
    ProfScope prof(p, 1, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(128), lds, st, planes, plane_stride, adv,
                       (const cx<T>*)p->tw, npairs, p->ldw, p->keep_cols > 0 ? p->keep_cols : 1024);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Row-pass kernel of a size.  5 = register-staged rows (default everywhere but 1024^2 fp64).
template <typename T, int N>
static constexpr int rows_default_version() {
    // 7 = cross-lane transforms (1024 points fp64): equal to 5 while the row pass streams from HBM (0.616 vs 0.607 ms
    // per launch on the whole batch) and ahead of it once the planes come from the Infinity Cache (chunked calls:
    // 7.54 vs 7.82 ms per step)
    // fp32 at 1024 points (round 6): 7 as well -- 1.36 against 2.08 ms per step of 64 fields at four waves per SIMD
    return N == 1024 ? 7 : 5;
}

template <typename T, int N>
static int launch_rows_advect(const tcfd_ns2d_plan* p, const cx<T>* planes, size_t plane_stride, cx<T>* adv, long batch,
                              hipStream_t st, int nyq = 0) {
    constexpr int EPT = Cfg<T, N>::ROW_EPT, THR = Cfg<T, N>::ROW_THREADS;
    if constexpr (!is_pow2c(N)) {
        // n = 3 * 2^k / 5 * 2^k: v5 (one plane per transform, next plane's rows in flight, one wave per SIMD); at 768^2 fp64 per
        // 7-field chunk launch: 43 us, against 53 for v3 (two planes per transform) and 124 for v5 capped at two waves per
        // SIMD (twelve complex fp64 per array spill there).  Only this one variant is instantiated for these sizes.
        return launch_rows_advect5<T, N, EPT, THR, 0, 1, 1>(p, planes, plane_stride, adv, batch, st, 0);
    } else {
    const bool split = use_split<T, N>(p);
    if constexpr (N == 128 || N == 256) {
        const int force = p->tune.small_tiles;
        if (!split && (force == 1 || (force != 0 && batch * (N / 2) < 16 * 256)))
            return launch_rows_advect5<T, N, 8, 64, 0, 1>(p, planes, plane_stride, adv, batch, st, nyq);
    }
    if constexpr (N == 1024 && sizeof(T) == 4) {
        if (p->tune.rows_v == 7 || p->tune.rows_v == 0) {   // cross-lane transforms in fp32 (half the registers of fp64: four waves
                                                            // per SIMD fit): per step at 1024^2 x 64 2.08 -> 1.36 ms against the Stockham rows
            if (p->tune.rows7_minw == 2) {
                if (split) return launch_rows_advect7<T, 1, 2, 1>(p, planes, plane_stride, adv, batch, st, nyq);
                return launch_rows_advect7<T, 0, 2, 1>(p, planes, plane_stride, adv, batch, st, nyq);
            }
            if (split) return launch_rows_advect7<T, 1, 4, 1>(p, planes, plane_stride, adv, batch, st, nyq);
            return launch_rows_advect7<T, 0, 4, 1>(p, planes, plane_stride, adv, batch, st, nyq);
        }
    }
    if constexpr (N == 1024 && sizeof(T) == 8) {
        if (p->tune.rows_v == 7 || p->tune.rows_v == 0) {   // cross-lane transforms: the default here
            if (split) return launch_rows_advect7<T, 1, 2, 1>(p, planes, plane_stride, adv, batch, st, nyq);
            return launch_rows_advect7<T, 0, 2, 1>(p, planes, plane_stride, adv, batch, st, nyq);
        }
        // v5 at this size: two waves per SIMD, rows loaded right before use (236 VGPRs, no spills)
        if (split) return launch_rows_advect5<T, N, EPT, THR, 1, 2, 0>(p, planes, plane_stride, adv, batch, st, nyq);
    }
    if constexpr (N >= 16) {
        if (split) return launch_rows_advect5<T, N, EPT, THR, 1, 1>(p, planes, plane_stride, adv, batch, st, nyq);
    }
    // 512-point fp32 rows: 164 registers with the packed arithmetic (tcfd_fft.hpp) -- three workgroups per CU (three waves per
    // SIMD) instead of one: the pass is bound by the latency of its dependent chains, not by issue (per step at 512^2 x 64:
    // 0.465 -> 0.352 ms, profiles/r06_rows_sweep.txt)
    if constexpr (N == 512 && sizeof(T) == 4)
        return launch_rows_advect5<T, N, EPT, THR, 0, 3>(p, planes, plane_stride, adv, batch, st, nyq);
    // ... and fp64 (240 registers): two per CU, 0.644 -> 0.587 ms per step (three: 0.80), profiles/r06_f64_rows_percu.txt
    if constexpr (N == 512 && sizeof(T) == 8)
        return launch_rows_advect5<T, N, EPT, THR, 0, 2>(p, planes, plane_stride, adv, batch, st, nyq);
    return launch_rows_advect5<T, N, EPT, THR, 0, 1>(p, planes, plane_stride, adv, batch, st, nyq);
    }
}

// ------------------------------------------------------------------ two batch halves, software pipelined
// The fused column pass saturates the HBM copy rate while the row pass is LDS / latency bound and leaves ~40 % of the
// read bandwidth idle.  The batch elements are independent, so the step is run on two half batches on two streams,
// half B one row pass behind half A: B's row pass then shares the chip with A's column pass and vice versa.
// (Experiment, off by default -- see step_impl.)
template <typename T, int N>
static int step_overlap_impl(const tcfd_ns2d_plan* p, const void* w_in, void* w_out, void* dwdt, long batch, int nstages,
                             const double* beta, const double* gdt, const double* mu, const double* fa,
                             const double* mud, const int* base0, int steps, double inv_total_dt, void* ws,
                             hipStream_t st, long ens_b0) {
    tcfd_ns2d_plan* mp = const_cast<tcfd_ns2d_plan*>(p);
    std::lock_guard<std::mutex> lock(mp->mu);   // the plan-owned streams / events serve one call at a time
    if (!mp->gs) mp->gs = new GraphState();
    GraphState* g = mp->gs;
    if (!g->stream) {
        HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g->ev_out, hipEventDisableTiming));
    }
    if (!g->stream2) {
        HIP_TRY(hipStreamCreateWithFlags(&g->stream2, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&g->ev_out2, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g->ev_rows, hipEventDisableTiming));
    }
    Ws<T> W = carve<T>(p, ws, batch);
    struct Half {
        ColArgs<T> a;
        const cx<T>* u_src; int u_src_ld;
        const cx<T>* w_in; cx<T>* w_out; cx<T>* dwdt;
        cx<T>* planes; cx<T>* adv; cx<T>* upad; cx<T>* upad2;
        long batch; hipStream_t q;
    } H[2];
    const long bA = batch / 2;
    for (int i = 0; i < 2; ++i) {
        const long b0 = i ? bA : 0;
        const size_t oc = (size_t)b0 * N * p->m, ow = (size_t)b0 * N * p->ldw;
        Half& h = H[i];
        h.batch = i ? batch - bA : bA;
        h.q = i ? g->stream2 : g->stream;
        h.w_in = (const cx<T>*)w_in + oc;
        h.w_out = (cx<T>*)w_out + oc;
        h.dwdt = dwdt ? (cx<T>*)dwdt + oc : nullptr;
        h.planes = W.planes + ow; h.adv = W.adv + ow; h.upad = W.upad + ow; h.upad2 = W.upad2 + ow;
        h.a = ColArgs<T>{};
        h.a.ens = ens_at<T>(p, ens_b0 + b0);
        h.a.nyq = p->nyq_a;
        h.a.planes = h.planes; h.a.plane_stride = W.plane_stride; h.a.h = W.h + ow; h.a.in = h.adv;
        h.a.u_in = h.w_in; h.a.u_in_ld = p->m;
        h.u_src = h.w_in; h.u_src_ld = p->m;
    }
    HIP_TRY(hipEventRecord(g->ev_in, st));
    int rc;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipStreamWaitEvent(H[i].q, g->ev_in, 0));
        if ((rc = launch_cols<T, N, MODE_A>(p, H[i].a, H[i].batch, H[i].q))) return rc;
        H[i].a.nyq = p->nyq_ca;
    }
    int planes_packed = p->nyq_a;
    auto cols = [&](Half& h, int k, bool last, const cx<T>* u0, int u0_ld) -> int {
        bool u0_needed_later = false;
        for (int k2 = k + 1; k2 < nstages; ++k2) u0_needed_later |= (base0 && base0[k2]);
        const bool from_u0 = base0 && base0[k];
        h.a.u_in = from_u0 ? u0 : h.u_src;
        h.a.u_in_ld = from_u0 ? u0_ld : h.u_src_ld;
        cx<T>* dst = h.upad;
        if (u0_needed_later && (const cx<T>*)dst == u0) dst = h.upad2;
        h.a.u_out = last ? h.w_out : dst;
        h.a.u_out_ld = last ? p->m : p->ldw;
        h.a.beta = (T)beta[k]; h.a.gdt = (T)gdt[k]; h.a.mu = (T)mu[k];
        h.a.fa = fa ? (T)fa[k] : (T)1;
        h.a.mud = mud ? (T)mud[k] : (T)mu[k];
        h.a.load_h = (k != 0);
        h.a.store_h = (k != nstages - 1);
        h.a.dwdt = last ? h.dwdt : nullptr;
        h.a.w0 = h.w_in;
        h.a.dwdt_scale = (T)inv_total_dt;
        int r = last ? launch_cols<T, N, MODE_C>(p, h.a, h.batch, h.q) : launch_cols<T, N, MODE_CA>(p, h.a, h.batch, h.q);
        h.u_src = h.a.u_out;
        h.u_src_ld = h.a.u_out_ld;
        return r;
    };
    for (int s = 0; s < steps; ++s) {
        const cx<T>* u0[2] = {H[0].u_src, H[1].u_src};
        const int u0_ld[2] = {H[0].u_src_ld, H[1].u_src_ld};
        for (int k = 0; k < nstages; ++k) {
            const bool last = (s == steps - 1) && (k == nstages - 1);
            if ((rc = launch_rows_advect<T, N>(p, H[0].planes, W.plane_stride, H[0].adv, H[0].batch, H[0].q, planes_packed))) return rc;
            HIP_TRY(hipEventRecord(g->ev_rows, H[0].q));
            HIP_TRY(hipStreamWaitEvent(H[1].q, g->ev_rows, 0));   // B stays one row pass behind A
            if ((rc = launch_rows_advect<T, N>(p, H[1].planes, W.plane_stride, H[1].adv, H[1].batch, H[1].q, planes_packed))) return rc;
            planes_packed = p->nyq_ca;
            if ((rc = cols(H[0], k, last, u0[0], u0_ld[0]))) return rc;
            if ((rc = cols(H[1], k, last, u0[1], u0_ld[1]))) return rc;
        }
    }
    HIP_TRY(hipEventRecord(g->ev_out, H[0].q));
    HIP_TRY(hipEventRecord(g->ev_out2, H[1].q));
    HIP_TRY(hipStreamWaitEvent(st, g->ev_out, 0));
    HIP_TRY(hipStreamWaitEvent(st, g->ev_out2, 0));
    return 0;
}

// ------------------------------------------------------------------ step driver
template <typename T, int N>
static int step_impl(const tcfd_ns2d_plan* p, const void* w_in, void* w_out, void* dwdt, long batch, int nstages,
                     const double* beta, const double* gdt, const double* mu, const double* fa, const double* mud,
                     const int* base0, int steps, double inv_total_dt, void* ws, hipStream_t st, long ens_b0) {
    {
        // opt-in (TCFD_OVERLAP=1): measured +2.6 % at 1024^2 x 64 fp64 -- both kernels fill the VGPR file, so the CUs
        // time-slice the two halves instead of co-running them; not worth two streams by default
        if (batch >= 2 && p->tune.overlap == 1)
            return step_overlap_impl<T, N>(p, w_in, w_out, dwdt, batch, nstages, beta, gdt, mu, fa, mud, base0, steps,
                                           inv_total_dt, ws, st, ens_b0);
    }
    Ws<T> W = carve<T>(p, ws, batch);
    int rc;
    ColArgs<T> a{};
    a.ens = ens_at<T>(p, ens_b0);
    a.planes = W.planes;
    a.plane_stride = W.plane_stride;
    a.h = W.h;
    a.in = W.adv;
    a.u_in = (const cx<T>*)w_in;
    a.u_in_ld = p->m;
    a.nyq = p->nyq_a;
    if ((rc = launch_cols<T, N, MODE_A>(p, a, batch, st))) return rc;
    int planes_packed = p->nyq_a;   // how the planes in the workspace were written: the row pass reads them that way
    cx<T>* h_cur = W.h;
    a.nyq = p->nyq_ca;
    // the caller's (n, m) rows are not 128-byte aligned (m is odd): only the first read and the last
    // write of a call touch that layout, every stage in between uses the aligned copy `upad`
    const cx<T>* u_src = (const cx<T>*)w_in;
    int u_src_ld = p->m;
    // one RK step on stream `q`; `first`/`final` select the caller-layout source / destination
    // General IMEX stage:  h <- fa_k F(u) + beta_k h ;  u <- (base + gdt_k h + mu_k L base) / (1 - mud_k L)  with
    // base = the current state, or (base0[k]) the state the step started from (IMEX RK2-CN, equations.py:190-228).
    // A stage whose successors still need the step's initial state writes to the second state buffer.
    auto run_step = [&](hipStream_t q, bool final) -> int {
        const cx<T>* u0 = u_src;
        const int u0_ld = u_src_ld;
        for (int k = 0; k < nstages; ++k) {
            int r;
            if ((r = launch_rows_advect<T, N>(p, W.planes, W.plane_stride, W.adv, batch, q, planes_packed))) return r;
            planes_packed = p->nyq_ca;
            const bool last = final && (k == nstages - 1);
            bool u0_needed_later = false;
            for (int k2 = k + 1; k2 < nstages; ++k2) u0_needed_later |= (base0 && base0[k2]);
            const bool from_u0 = base0 && base0[k];
            a.u_in = from_u0 ? u0 : u_src;
            a.u_in_ld = from_u0 ? u0_ld : u_src_ld;
            cx<T>* dst = W.upad;
            if (u0_needed_later && (const cx<T>*)dst == u0) dst = W.upad2;
            a.u_out = last ? (cx<T>*)w_out : dst;
            a.u_out_ld = last ? p->m : p->ldw;
            a.beta = (T)beta[k];
            a.gdt = (T)gdt[k];
            a.mu = (T)mu[k];
            a.fa = fa ? (T)fa[k] : (T)1;
            a.mud = mud ? (T)mud[k] : (T)mu[k];
            a.load_h = (k != 0);  // h starts from 0 every step (equations.py:353)
            a.store_h = (k != nstages - 1);
            a.h = h_cur;
            a.h_out = h_cur;
            a.dwdt = last ? (cx<T>*)dwdt : nullptr;
            a.w0 = (const cx<T>*)w_in;
            a.dwdt_scale = (T)inv_total_dt;
            r = last ? launch_cols<T, N, MODE_C>(p, a, batch, q) : launch_cols<T, N, MODE_CA>(p, a, batch, q);
            if (r) return r;
            u_src = a.u_out;
            u_src_ld = a.u_out_ld;
            h_cur = a.h_out;
        }
        return 0;
    };
    const long state_bytes = (long)batch * N * p->ldw * (long)sizeof(cx<T>);
    const int graph_env = p->tune.graph;
    const bool profiling = p->prof && p->prof->on;
    const bool use_graph = steps >= 3 && !profiling &&
                           graph_env == 1;   // opt-in since round 4 (plain launches are faster at every size measured)
    (void)state_bytes;
    int s0 = 0;
    if (use_graph) {
        tcfd_ns2d_plan* mp = const_cast<tcfd_ns2d_plan*>(p);
        // the captured graph, its stream and its fence events are plan-owned and mutable: host threads that share a
        // plan take turns here (the replays of one call are enqueued before the next call may re-capture)
        std::lock_guard<std::mutex> lock(mp->mu);
        if (!mp->gs) mp->gs = new GraphState();
        GraphState* g = mp->gs;
        if (!g->stream) {
            HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&g->ev_out, hipEventDisableTiming));
        }
        if ((rc = run_step(st, false))) return rc;   // step 1: caller layout -> upad (also sets every kernel attribute)
        std::vector<double> coef;
        for (int k = 0; k < nstages; ++k) {
            coef.push_back(beta[k]); coef.push_back(gdt[k]); coef.push_back(mu[k]);
            coef.push_back(fa ? fa[k] : 1.0); coef.push_back(mud ? mud[k] : mu[k]); coef.push_back(base0 ? base0[k] : 0);
        }
        auto capture = [&](int reps, hipGraph_t* graph, hipGraphExec_t* exec) -> int {
            HIP_TRY(hipStreamBeginCapture(g->stream, hipStreamCaptureModeThreadLocal));
            int r = 0;
            for (int i = 0; i < reps && !r; ++i) r = run_step(g->stream, false);         // upad -> upad
            hipError_t e = hipStreamEndCapture(g->stream, graph);
            if (r) return r;
            if (e != hipSuccess) return fail(TCFD_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
            HIP_TRY(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
            return 0;
        };
        // (the captured launches hold the chunk's slice of the ensemble table: another chunk, or a table set anew, is another graph)
        if (!g->exec || g->batch != batch || g->nstages != nstages || g->ws != ws || g->coef != coef || g->ens != (const void*)a.ens) {
            if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
            if (g->graph) { (void)hipGraphDestroy(g->graph); g->graph = nullptr; }
            if (g->exec_multi) { (void)hipGraphExecDestroy(g->exec_multi); g->exec_multi = nullptr; }
            if (g->graph_multi) { (void)hipGraphDestroy(g->graph_multi); g->graph_multi = nullptr; }
            if ((rc = capture(1, &g->graph, &g->exec))) return rc;
            g->batch = batch; g->nstages = nstages; g->ws = ws; g->coef = coef; g->ens = a.ens;
        }
        int interior = steps - 2;
        if (interior >= 2 * GraphState::MULTI && !g->exec_multi &&
            (rc = capture(GraphState::MULTI, &g->graph_multi, &g->exec_multi)))
            return rc;
        HIP_TRY(hipEventRecord(g->ev_in, st));
        HIP_TRY(hipStreamWaitEvent(g->stream, g->ev_in, 0));
        if (g->exec_multi)
            for (; interior >= GraphState::MULTI; interior -= GraphState::MULTI)
                HIP_TRY(hipGraphLaunch(g->exec_multi, g->stream));
        for (; interior > 0; --interior) HIP_TRY(hipGraphLaunch(g->exec, g->stream));
        HIP_TRY(hipEventRecord(g->ev_out, g->stream));
        HIP_TRY(hipStreamWaitEvent(st, g->ev_out, 0));
        s0 = steps - 1;
    }
    for (int s = s0; s < steps; ++s)
        if ((rc = run_step(st, s == steps - 1))) return rc;
    return 0;
}

template <typename T, int N>
static int explicit_impl(const tcfd_ns2d_plan* p, const void* w, void* out, const void* wt, void* psi, bool residual,
                         long batch, void* ws, hipStream_t st, long ens_b0) {
    Ws<T> W = carve<T>(p, ws, batch);
    int rc;
    ColArgs<T> a{};
    a.ens = ens_at<T>(p, ens_b0);
    a.planes = W.planes;
    a.plane_stride = W.plane_stride;
    a.u_in = (const cx<T>*)w;
    a.u_in_ld = p->m;
    if ((rc = launch_cols<T, N, MODE_A>(p, a, batch, st))) return rc;
    if ((rc = launch_rows_advect<T, N>(p, W.planes, W.plane_stride, W.adv, batch, st))) return rc;
    a.in = W.adv;
    a.out = (cx<T>*)out;
    if (residual) {
        a.wt = (const cx<T>*)wt;
        a.psi = (cx<T>*)psi;
        return launch_cols<T, N, MODE_RES>(p, a, batch, st);
    }
    return launch_cols<T, N, MODE_F>(p, a, batch, st);
}

template <typename T, int N>
static int rfft2_impl(const tcfd_ns2d_plan* p, const void* x, void* out, long batch, hipStream_t st) {
    using Gm = RowGeom<T, N, Cfg<T, N>::ROW_EPT>;
    auto kern = k_rows_r2c<T, N, Cfg<T, N>::ROW_EPT>;
    static DevOnce lds_once;
    if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
    const long npairs = batch * (N / 2);
    const long blocks = (npairs + Gm::GROUPS - 1) / Gm::GROUPS;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const T*)x, (cx<T>*)out,
                       (const cx<T>*)p->tw, npairs, p->m);
    HIP_TRY(hipGetLastError());
    ColArgs<T> a{};
    a.in = (const cx<T>*)out;
    a.out = (cx<T>*)out;
    a.in_ld = a.out_ld = p->m;
    a.scale = (T)1;
    return launch_cols<T, N, MODE_FWD>(p, a, batch, st);
}

template <typename T, int N>
static int irfft2_impl(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, void* ws, hipStream_t st) {
    ColArgs<T> a{};
    a.in = (const cx<T>*)xh;
    a.out = (cx<T>*)ws;
    a.in_ld = p->m;
    a.out_ld = p->ldw;
    a.scale = (T)1 / ((T)N * (T)N);
    int rc;
    if ((rc = launch_cols<T, N, MODE_INV>(p, a, batch, st))) return rc;
    using Gm = RowGeom<T, N, Cfg<T, N>::ROW_EPT>;
    auto kern = k_rows_c2r<T, N, Cfg<T, N>::ROW_EPT>;
    static DevOnce lds_once;
    {
        rc = set_lds(lds_once, kern, Gm::LDS_BYTES);
        if (rc) return rc;
    }
    const long npairs = batch * (N / 2);
    const long blocks = (npairs + Gm::GROUPS - 1) / Gm::GROUPS;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const cx<T>*)ws, (T*)out,
                       (const cx<T>*)p->tw, npairs, p->ldw);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T, int N>
static int irfft2_sub_impl(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, int S, void* ws, hipStream_t st) {
    using Gm = RowGeom<T, N, Cfg<T, N>::ROW_EPT>;
    if (S < 2 || (S & (S - 1)) || S > Gm::G || S > 64)
        return fail(TCFD_EINVAL, "irfft2_subsample: factor %d is not a power of two in [2, %d] (n = %d)", S, Gm::G < 64 ? Gm::G : 64, N);
    ColArgs<T> a{};
    a.in = (const cx<T>*)xh;
    a.out = (cx<T>*)ws;
    a.in_ld = p->m;
    a.out_ld = p->ldw;
    a.scale = (T)1 / ((T)N * (T)N);
    int rc;
    if ((rc = launch_cols<T, N, MODE_INV>(p, a, batch, st))) return rc;
    auto kern = k_rows_c2r_sub<T, N, Cfg<T, N>::ROW_EPT>;
    static DevOnce lds_once;
    {
        rc = set_lds(lds_once, kern, Gm::LDS_BYTES);
        if (rc) return rc;
    }
    const long nrows = batch * (N / S);
    const long blocks = (nrows + Gm::GROUPS - 1) / Gm::GROUPS;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const cx<T>*)ws, (T*)out,
                       (const cx<T>*)p->tw, nrows, p->ldw, S);
    HIP_TRY(hipGetLastError());
    return 0;
}

// n = 3 * 2^k: how many fields make ONE round of resident column workgroups.  These plans run whole-column Stockham tiles
// (768^2 fp64: 107 KB of LDS = one 512-lane workgroup per CU, 49 tiles per field): a cache-sized chunk of 7 fields is 343
// workgroups = 1.34 rounds, 5 fields are 245 = one round -- 157 -> 181 steps/s.
template <typename T, int N>
static int round_fields_impl(tcfd_ns2d_plan* p) {
    if constexpr (is_pow2c(N)) {
        p->tune.round_fields = 0;
    } else {
        constexpr int EPT = Cfg<T, N>::COL_EPT, C = Cfg<T, N>::COLS;
        constexpr size_t lds = (size_t)lds_elems<N, EPT, C, false>() * sizeof(cx<T>) + 3 * (size_t)N * sizeof(T);
        constexpr int threads = C * (N / EPT);
        const int by_lds = (int)std::max<size_t>(1, (160 * 1024) / lds), by_thr = std::max(1, 1024 / threads);
        const int per_cu = std::min(std::min(by_lds, by_thr), 2);      // the column kernels use > 128 registers at EPT = 12
        const int tiles = (p->m + C - 1) / C;
        p->tune.round_fields = std::max(1, 256 * per_cu / tiles);
    }
    return 0;
}

// Vector-Jacobian product of the explicit terms (the backward of tcfd_ns2d_explicit_terms): from the state w and the
// pre-weighted cotangent gm = mask * g / c it produces the four half spectra  X_f = rfft2(Y_f)  (k_rows_vjp), which the caller
// combines:  wbar = -(c / n^2) sum_f conj(a_f) X_f.  Three kinds of launches per chunk: the opening column pass of the forward
// (w -> 4 planes) + the column inverse transform of gm, the row pass above, four generic column forward transforms.
template <typename T, int N>
static int explicit_vjp_impl(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, size_t x_field_stride,
                             long batch, void* ws, hipStream_t st) {
    Ws<T> W = carve<T>(p, ws, batch);
    int rc;
    ColArgs<T> a{};
    a.planes = W.planes;
    a.plane_stride = W.plane_stride;
    a.u_in = (const cx<T>*)w;
    a.u_in_ld = p->m;
    a.nyq = 0;    // whole-column tiles, every column present (the row pass reads the plain layout)
    if ((rc = launch_cols_v<T, N, MODE_A, Cfg<T, N>::COL_EPT, Cfg<T, N>::COLS>(p, a, batch, st))) return rc;
    ColArgs<T> g{};
    g.in = (const cx<T>*)gm;
    g.out = W.adv;
    g.in_ld = p->m;
    g.out_ld = p->ldw;
    g.scale = (T)1;
    if ((rc = launch_cols<T, N, MODE_INV>(p, g, batch, st))) return rc;
    {
        constexpr int EPT = Cfg<T, N>::ROW_EPT, THR = Cfg<T, N>::ROW_THREADS;
        using Gm = RowGeom<T, N, EPT, THR>;
        auto kern = k_rows_vjp<T, N, EPT, THR>;
        static DevOnce lds_once;
        if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
        const long npairs = batch * (N / 2);
        const long blocks = rows_grid(p, (npairs + Gm::GROUPS - 1) / Gm::GROUPS, 4);
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, W.planes, W.plane_stride,
                           (const cx<T>*)W.adv, (const cx<T>*)p->tw, npairs, p->ldw);
        HIP_TRY(hipGetLastError());
    }
    for (int f = 0; f < 4; ++f) {
        ColArgs<T> c{};
        c.in = W.planes + (size_t)f * W.plane_stride;
        c.out = (cx<T>*)xout + (size_t)f * x_field_stride;
        c.in_ld = p->ldw;
        c.out_ld = p->m;
        c.scale = (T)1;
        if ((rc = launch_cols<T, N, MODE_FWD>(p, c, batch, st))) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ tangent-linear model (forward-mode JVP)
// F'(w) dw = M . R( -(ddxw u + dxw du + ddyw v + dyw dv) ),  d-fields = I(a_f dw): no forcing term.  Per chunk: the opening
// column pass twice (w and dw -> two sets of four planes, plain layout, whole-column tiles as explicit_vjp_impl), ONE row pass
// (k_rows_jvp) that carries both through the advection, the closing column pass for p (mask + forcing) and for dp (mask only).
// Scratch: JvpWs (tcfd_ns2d_plan.hpp).  F and dF of a stage land in plane 0 of their sets (the planes are dead after the row pass).

// Sizes whose one-pass row kernel would need scratch memory run p and dp as two row passes: the fp64 transforms of 20
// elements per lane (n = 5 * 2^k), where four arrays are 320 registers before the radix-20 butterfly's temporaries (one pass:
// 128 - 692 bytes of scratch per lane; the two passes: none -- profiles/ns2d_jvp_kernel_resource_usage.txt).
template <typename T, int N>
static constexpr bool jvp_two_pass() {
    return sizeof(T) == 8 && Cfg<T, N>::ROW_EPT == 20;
}

template <typename T, int N, int PART>
static int launch_rows_jvp(const tcfd_ns2d_plan* p, const JvpWs<T>& W, long batch, hipStream_t st) {
    constexpr int EPT = Cfg<T, N>::ROW_EPT, THR = Cfg<T, N>::ROW_THREADS;
    using Gm = RowGeom<T, N, EPT, THR>;
    auto kern = k_rows_jvp<T, N, EPT, THR, PART>;
    static DevOnce lds_once;
    if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
    const long npairs = batch * (N / 2);
    const long blocks = rows_grid(p, (npairs + Gm::GROUPS - 1) / Gm::GROUPS, 4);
    ProfScope prof(p, 1, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const cx<T>*)W.planes,
                       (const cx<T>*)W.dplanes, W.plane_stride, W.adv, W.dadv, (const cx<T>*)p->tw, npairs, p->ldw);
    HIP_TRY(hipGetLastError());
    return 0;
}

// out_f may be null (the caller wants the tangent only); out_f / out_df: caller layout (pitch m)
template <typename T, int N>
static int explicit_jvp_impl(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df, long batch,
                             void* ws, hipStream_t st) {
    constexpr int CEPT = Cfg<T, N>::COL_EPT, COLS = Cfg<T, N>::COLS;
    JvpWs<T> W = carve_jvp<T>(p, ws, batch);
    int rc;
    ColArgs<T> a{};
    a.plane_stride = W.plane_stride;
    a.u_in_ld = p->m;
    a.nyq = 0;    // whole-column tiles, every column present (the row pass reads the plain layout)
    a.planes = W.planes;
    a.u_in = (const cx<T>*)w;
    if ((rc = launch_cols_v<T, N, MODE_A, CEPT, COLS>(p, a, batch, st))) return rc;
    a.planes = W.dplanes;
    a.u_in = (const cx<T>*)dw;
    if ((rc = launch_cols_v<T, N, MODE_A, CEPT, COLS>(p, a, batch, st))) return rc;
    if constexpr (jvp_two_pass<T, N>()) {
        if (out_f && (rc = launch_rows_jvp<T, N, 1>(p, W, batch, st))) return rc;
        if ((rc = launch_rows_jvp<T, N, 2>(p, W, batch, st))) return rc;
    } else {
        if ((rc = launch_rows_jvp<T, N, 0>(p, W, batch, st))) return rc;
    }
    ColArgs<T> c{};
    if (out_f) {
        c.in = W.adv;
        c.out = (cx<T>*)out_f;
        if ((rc = launch_cols_v<T, N, MODE_F, CEPT, COLS>(p, c, batch, st))) return rc;
    }
    c.in = W.dadv;
    c.out = (cx<T>*)out_df;
    return launch_cols_v<T, N, MODE_F, CEPT, COLS>(p, c, batch, st, /*no_forcing=*/true);
}

// The stage update on the state and on the tangent in one launch: k_stage_update's arithmetic on both (the update is linear,
// and the tangent sees no forcing).  hp / dhp null: first stage of a step (h starts from 0); h / dh null: last stage (nothing
// reads the accumulator).  b may be u (in-place update of a state buffer: every element is read before it is written, by the
// same thread) -- hence no __restrict__ on the state and accumulator pointers.
template <typename T>
__global__ __launch_bounds__(256) void k_stage_update_jvp(const cx<T>* __restrict__ f, const cx<T>* __restrict__ df,
                                                          const cx<T>* hp, const cx<T>* dhp, const cx<T>* b, const cx<T>* db,
                                                          const T* __restrict__ Lt, T fa, T beta, T gdt, T mu, T mud, cx<T>* h,
                                                          cx<T>* dh, cx<T>* u, cx<T>* du, long total, long plane) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const T L = Lt[e % plane];
        const T r = fast_rcp((T)1 - mud * L);
        cx<T> hn = cscale(f[e], fa), dhn = cscale(df[e], fa);
        if (hp) {
            hn = hn + cscale(hp[e], beta);
            dhn = dhn + cscale(dhp[e], beta);
        }
        const cx<T> bv = b[e], dbv = db[e];
        const cx<T> rhs = bv + cscale(hn, gdt) + cscale(cscale(bv, L), mu);
        const cx<T> drhs = dbv + cscale(dhn, gdt) + cscale(cscale(dbv, L), mu);
        if (h) {
            h[e] = hn;
            dh[e] = dhn;
        }
        u[e] = cscale(rhs, r);
        du[e] = cscale(drhs, r);
    }
}

// `steps` steps of the schedule of tcfd_ns2d_step_imex on the pair (w, dw): per stage the sweep above, then the stage update
template <typename T, int N>
static int step_jvp_impl(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out, long batch,
                         int nstages, const double* fa, const double* beta, const double* gdt, const double* mu,
                         const double* mud, const int* base0, int steps, void* ws, hipStream_t st) {
    JvpWs<T> W = carve_jvp<T>(p, ws, batch);
    const long plane = (long)N * p->m, total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    const cx<T>* u_src = (const cx<T>*)w_in;
    const cx<T>* du_src = (const cx<T>*)dw_in;
    cx<T>* F = W.planes;     // plane 0 of each set: free once the row pass has run
    cx<T>* dF = W.dplanes;
    for (int s = 0; s < steps; ++s) {
        const cx<T>* u0 = u_src;
        const cx<T>* du0 = du_src;
        for (int k = 0; k < nstages; ++k) {
            int rc;
            if ((rc = explicit_jvp_impl<T, N>(p, u_src, du_src, F, dF, batch, ws, st))) return rc;
            const bool last = (s == steps - 1) && (k == nstages - 1);
            bool u0_needed_later = false;
            for (int k2 = k + 1; k2 < nstages; ++k2) u0_needed_later |= (base0 && base0[k2]);
            const bool from_u0 = base0 && base0[k];
            int d = 0;
            if (u0_needed_later && (const cx<T>*)W.s[0] == u0) d = 1;
            cx<T>* out = last ? (cx<T>*)w_out : W.s[d];
            cx<T>* dout = last ? (cx<T>*)dw_out : W.ds[d];
            const bool load_h = (k != 0), store_h = (k != nstages - 1);   // h starts from 0 every step
            hipLaunchKernelGGL(k_stage_update_jvp<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)F, (const cx<T>*)dF,
                               load_h ? (const cx<T>*)W.h : nullptr, load_h ? (const cx<T>*)W.dh : nullptr,
                               from_u0 ? u0 : u_src, from_u0 ? du0 : du_src, (const T*)p->lin, fa ? (T)fa[k] : (T)1, (T)beta[k],
                               (T)gdt[k], (T)mu[k], mud ? (T)mud[k] : (T)mu[k], store_h ? W.h : nullptr,
                               store_h ? W.dh : nullptr, out, dout, total, plane);
            HIP_TRY(hipGetLastError());
            u_src = out;
            du_src = dout;
        }
    }
    return 0;
}

// ------------------------------------------------------------------ tangent bundle: one state, K tangents
// The sweep of explicit_jvp_impl with the state's share done once: MODE_A on w, then group by group (kg tangents, bundle_shape in
// tcfd_ns2d.hip) MODE_A on the group's tangents, ONE row pass for the group (k_rows_jvp_bundle; the first group's also writes p),
// MODE_F on p and on the group's dp.  A group's planes are [plane][tangent][field], so its column passes are single launches
// over kg * batch fields wherever the tangents are tangent_stride == batch fields apart (always inside a step; at the call's
// edges when the call is one chunk).

// Sizes that run the two-pass row kernels instead (k_rows_jvp PART = 1 once, PART = 2 per tangent -- the state's planes are read
// again per tangent, but nothing of the state is repeated in the column passes or the stage update): those whose stash leaves a
// CU fewer than two workgroups.  A workgroup is one wave or one group, and holds 5 EPT elements of LDS per lane; above 80 KB one
// workgroup -- one or two waves -- would own the CU's 160 KB alone and nothing would hide its transforms' exchange latency.
// fp64: n = 5 * 2^k (20 elements per lane, 100 KB), 1536 (120 KB), 2048 (160 KB), 4096 (320 KB: not launchable); fp32: 4096 (160 KB).
template <typename T, int N>
static constexpr bool bundle_two_pass() {
    return BundleGeom<T, N, Cfg<T, N>::ROW_EPT>::LDS_BYTES > 80 * 1024;
}
// TCFD_BUNDLE_ROWS = 0 runs the two-pass form at every size (the A/B that DESIGN 23 records)
template <typename T, int N>
static bool bundle_runs_two_pass(const tcfd_ns2d_plan* p) {
    return bundle_two_pass<T, N>() || p->tune.bundle_rows == 0;
}

template <typename T, int N>
static int launch_rows_jvp_bundle(const tcfd_ns2d_plan* p, const BundleWs<T>& W, bool want_p, int ntan, long batch, hipStream_t st) {
    if (bundle_runs_two_pass<T, N>(p)) {
        JvpWs<T> J{};
        J.planes = W.planes;
        J.adv = W.adv;
        J.plane_stride = W.plane_stride;
        int rc;
        if (want_p && (rc = launch_rows_jvp<T, N, 1>(p, J, batch, st))) return rc;
        // PART = 2 reads the four planes of ONE tangent plane_stride apart: [tangent][plane] within the group here
        for (int t = 0; t < ntan; ++t) {
            J.dplanes = W.dplanes + (size_t)t * 4 * W.plane_stride;
            J.dadv = W.dadv + (size_t)t * W.plane_stride;
            if ((rc = launch_rows_jvp<T, N, 2>(p, J, batch, st))) return rc;
        }
        return 0;
    }
    if constexpr (!bundle_two_pass<T, N>()) {
        constexpr int EPT = Cfg<T, N>::ROW_EPT;
        using Gm = BundleGeom<T, N, EPT>;
        auto kern = k_rows_jvp_bundle<T, N, EPT>;
        static DevOnce lds_once;
        if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
        const long npairs = batch * (N / 2);
        const int per_cu = (int)std::min<size_t>(16, (160 * 1024) / Gm::LDS_BYTES);   // workgroups a CU holds
        const long blocks = rows_grid(p, (npairs + Gm::GROUPS - 1) / Gm::GROUPS, 2 * per_cu);
        // A small problem has fewer row pairs than the device has workgroup slots, and a group folds its K tangents one after
        // the other: the tangents are then cut into segments (blockIdx.y), each redoing the state's four transforms, until the
        // slots are filled (256^2 x 2 fp64: 64 workgroups of 36 transforms -> 512 of 8).  The arithmetic of a member is the same
        // in any segment, so the bits do not depend on the cut.
        const long slots = 256L * per_cu;
        const int segs = (int)std::max<long>(1, std::min<long>(ntan, slots / blocks));
        ProfScope prof(p, 1, st);
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)segs), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const cx<T>*)W.planes,
                           W.plane_stride, (const cx<T>*)W.dplanes, W.dplane_stride, W.plane_stride, want_p ? W.adv : nullptr,
                           W.dadv, W.plane_stride, (const cx<T>*)p->tw, npairs, p->ldw, ntan);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// w: batch fields; dw / out_df: ntan tangents of batch fields, in_ts / out_ts elements apart (caller layout, pitch m); out_f may be null
template <typename T, int N>
static int explicit_jvp_bundle_impl(const tcfd_ns2d_plan* p, const BundleWs<T>& W, const cx<T>* w, const cx<T>* dw, size_t in_ts,
                                    cx<T>* out_f, cx<T>* out_df, size_t out_ts, long batch, int ntan, int kg, hipStream_t st) {
    constexpr int CEPT = Cfg<T, N>::COL_EPT, COLS = Cfg<T, N>::COLS;
    const bool TWO = bundle_runs_two_pass<T, N>(p);
    const size_t tight = (size_t)batch * N * p->m;                           // tangents one after the other, caller layout
    const bool ws_tight = W.plane_stride == (size_t)batch * N * p->ldw;     // a field's scratch is not padded
    int rc;
    ColArgs<T> a{};
    a.plane_stride = W.plane_stride;
    a.u_in_ld = p->m;
    a.nyq = 0;    // whole-column tiles, every column present (the row passes read the plain layout)
    a.planes = W.planes;
    a.u_in = w;
    if ((rc = launch_cols_v<T, N, MODE_A, CEPT, COLS>(p, a, batch, st))) return rc;
    for (int k0 = 0; k0 < ntan; k0 += kg) {
        const int kn = std::min(kg, ntan - k0);
        const bool first = (k0 == 0), want_p = first && out_f;
        // the group's planes: [plane][tangent][field] (two-pass sizes: [tangent][plane][field], what k_rows_jvp reads)
        a.plane_stride = TWO ? W.plane_stride : W.dplane_stride;
        if (!TWO && ws_tight && in_ts == tight) {
            a.planes = W.dplanes;
            a.u_in = dw + (size_t)k0 * in_ts;
            if ((rc = launch_cols_v<T, N, MODE_A, CEPT, COLS>(p, a, (long)kn * batch, st))) return rc;
        } else {
            for (int t = 0; t < kn; ++t) {
                a.planes = W.dplanes + (size_t)t * (TWO ? 4 : 1) * W.plane_stride;
                a.u_in = dw + (size_t)(k0 + t) * in_ts;
                if ((rc = launch_cols_v<T, N, MODE_A, CEPT, COLS>(p, a, batch, st))) return rc;
            }
        }
        if ((rc = launch_rows_jvp_bundle<T, N>(p, W, want_p, kn, batch, st))) return rc;
        ColArgs<T> c{};
        if (want_p) {
            c.in = W.adv;
            c.out = out_f;
            if ((rc = launch_cols_v<T, N, MODE_F, CEPT, COLS>(p, c, batch, st))) return rc;
        }
        if (ws_tight && out_ts == tight) {
            c.in = W.dadv;
            c.out = out_df + (size_t)k0 * out_ts;
            if ((rc = launch_cols_v<T, N, MODE_F, CEPT, COLS>(p, c, (long)kn * batch, st, /*no_forcing=*/true))) return rc;
        } else {
            for (int t = 0; t < kn; ++t) {
                c.in = W.dadv + (size_t)t * W.plane_stride;
                c.out = out_df + (size_t)(k0 + t) * out_ts;
                if ((rc = launch_cols_v<T, N, MODE_F, CEPT, COLS>(p, c, batch, st, /*no_forcing=*/true))) return rc;
            }
        }
    }
    return 0;
}

// The stage update on the state (member 0) and on the K tangents (members 1 .. K) in one launch: k_stage_update_jvp's arithmetic,
// member by member (blockIdx.y strides over the members).  Tangent arrays are `*_ts` elements apart.  Null hp / h as there; b may
// be u (in place) -- no __restrict__ on the state and accumulator pointers.
template <typename T>
struct StageBundleArgs {
    const cx<T>* f; const cx<T>* df; size_t df_ts;
    const cx<T>* hp; const cx<T>* dhp;
    const cx<T>* b; const cx<T>* db; size_t db_ts;
    cx<T>* h; cx<T>* dh; size_t dh_ts;
    cx<T>* u; cx<T>* du; size_t du_ts;
    const T* Lt;
    T fa, beta, gdt, mu, mud;
    long total, plane;
    int ntan;
};
template <typename T>
__global__ __launch_bounds__(256) void k_stage_update_bundle(StageBundleArgs<T> a) {
    for (int mem = blockIdx.y; mem <= a.ntan; mem += gridDim.y) {
        const size_t k = mem ? (size_t)(mem - 1) : 0;
        const cx<T>* f = mem ? a.df + k * a.df_ts : a.f;
        const cx<T>* hp = !a.hp ? nullptr : (mem ? a.dhp + k * a.dh_ts : a.hp);
        const cx<T>* b = mem ? a.db + k * a.db_ts : a.b;
        cx<T>* h = !a.h ? nullptr : (mem ? a.dh + k * a.dh_ts : a.h);
        cx<T>* u = mem ? a.du + k * a.du_ts : a.u;
        for (long e = blockIdx.x * 256L + threadIdx.x; e < a.total; e += (long)gridDim.x * 256L) {
            const T L = a.Lt[e % a.plane];
            const T r = fast_rcp((T)1 - a.mud * L);
            cx<T> hn = cscale(f[e], a.fa);
            if (hp) hn = hn + cscale(hp[e], a.beta);
            const cx<T> bv = b[e];
            const cx<T> rhs = bv + cscale(hn, a.gdt) + cscale(cscale(bv, L), a.mu);
            if (h) h[e] = hn;
            u[e] = cscale(rhs, r);
        }
    }
}

template <typename T, int N>
static int explicit_jvp_bundle_entry(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df,
                                     size_t tan_stride, long batch, int ntan, int kg, void* ws, hipStream_t st) {
    const BundleWs<T> W = carve_bundle<T>(p, ws, batch, ntan, kg);
    return explicit_jvp_bundle_impl<T, N>(p, W, (const cx<T>*)w, (const cx<T>*)dw, tan_stride, (cx<T>*)out_f, (cx<T>*)out_df,
                                          tan_stride, batch, ntan, kg, st);
}

// `steps` steps of the schedule of tcfd_ns2d_step_imex on the state and its K tangents: step_jvp_impl's sequencing, the tangent
// buffers K deep.  dh_k starts from 0 every step, as h does.
template <typename T, int N>
static int step_jvp_bundle_impl(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out,
                                size_t tan_stride, long batch, int ntan, int kg, int nstages, const double* fa, const double* beta,
                                const double* gdt, const double* mu, const double* mud, const int* base0, int steps, void* ws,
                                hipStream_t st) {
    const BundleWs<T> W = carve_bundle<T>(p, ws, batch, ntan, kg);
    const long plane = (long)N * p->m, total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    const unsigned members = (unsigned)std::min(ntan + 1, 1024);
    const cx<T>* u_src = (const cx<T>*)w_in;
    const cx<T>* du_src = (const cx<T>*)dw_in;
    size_t du_ts = tan_stride;
    for (int s = 0; s < steps; ++s) {
        const cx<T>* u0 = u_src;
        const cx<T>* du0 = du_src;
        const size_t du0_ts = du_ts;
        for (int k = 0; k < nstages; ++k) {
            int rc;
            if ((rc = explicit_jvp_bundle_impl<T, N>(p, W, u_src, du_src, du_ts, W.F, W.dF, W.tan_stride, batch, ntan, kg, st)))
                return rc;
            const bool last = (s == steps - 1) && (k == nstages - 1);
            bool u0_needed_later = false;
            for (int k2 = k + 1; k2 < nstages; ++k2) u0_needed_later |= (base0 && base0[k2]);
            const bool from_u0 = base0 && base0[k];
            int d = 0;
            if (u0_needed_later && (const cx<T>*)W.s[0] == u0) d = 1;
            const bool load_h = (k != 0), store_h = (k != nstages - 1);   // h starts from 0 every step
            StageBundleArgs<T> a{};
            a.f = W.F; a.df = W.dF; a.df_ts = W.tan_stride;
            a.hp = load_h ? W.h : nullptr; a.dhp = W.dh;
            a.b = from_u0 ? u0 : u_src; a.db = from_u0 ? du0 : du_src; a.db_ts = from_u0 ? du0_ts : du_ts;
            a.h = store_h ? W.h : nullptr; a.dh = W.dh; a.dh_ts = W.tan_stride;
            a.u = last ? (cx<T>*)w_out : W.s[d];
            a.du = last ? (cx<T>*)dw_out : W.ds[d];
            a.du_ts = last ? tan_stride : W.tan_stride;
            a.Lt = (const T*)p->lin;
            a.fa = fa ? (T)fa[k] : (T)1; a.beta = (T)beta[k]; a.gdt = (T)gdt[k]; a.mu = (T)mu[k]; a.mud = mud ? (T)mud[k] : (T)mu[k];
            a.total = total; a.plane = plane; a.ntan = ntan;
            hipLaunchKernelGGL(k_stage_update_bundle<T>, dim3(blocks, members), dim3(256), 0, st, a);
            HIP_TRY(hipGetLastError());
            u_src = a.u;
            du_src = a.du;
            du_ts = a.du_ts;
        }
    }
    return 0;
}

// ------------------------------------------------------------------ adjoint model (reverse of the fused step)
// Reverse of stage k of the schedule, everything that is element-wise (the transposes of k_stage_update, of the `g * pre`
// weighting and of the additions autograd performs between its nodes), one launch:
//     g = r (.) ubar_{k+1} ,  G = hbar_k + gdt g ,  gm = pre (.) fa G ,  hbar_{k-1} = beta G ,  bbar = (1 + mu L) g ,  r = 1 / (1 - mud L)
// ub / hb null: a zero cotangent (hbar is zero at the last stage of every step).  hprev null: first stage, nobody reads it.  bbar
// is the cotangent of the stage's base state: of u_k (-> acc, which the closing kernel completes to ubar_k), or, when `ustart` is
// given (a base0 stage), of the step's initial state (-> ustart, stored or added; acc = 0).  acc may be ub and hprev may be hb
// (every element is read before it is written, by the same thread) -- hence no __restrict__ on them.
template <typename T>
__global__ __launch_bounds__(256) void k_stage_adjoint(const cx<T>* ub, const cx<T>* hb, const T* __restrict__ Lt,
                                                       const T* __restrict__ pre, T fa, T beta, T gdt, T mu, T mud,
                                                       cx<T>* __restrict__ gm, cx<T>* hprev, cx<T>* acc, cx<T>* ustart,
                                                       int ustart_add, long total, long plane) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long t = e % plane;
        const T L = Lt[t];
        cx<T> g = mk<T>((T)0, (T)0);
        if (ub) g = cscale(ub[e], fast_rcp((T)1 - mud * L));
        cx<T> G = cscale(g, gdt);
        if (hb) G = G + hb[e];
        gm[e] = cscale(cscale(G, fa), pre[t]);
        if (hprev) hprev[e] = cscale(G, beta);
        const cx<T> bb = g + cscale(cscale(g, L), mu);
        if (ustart) {
            ustart[e] = ustart_add ? ustart[e] + bb : bb;
            acc[e] = mk<T>((T)0, (T)0);
        } else {
            acc[e] = bb;
        }
    }
}

// ubar_k = acc + sum_f post_f (.) X_f [+ extra]: the closing sum of the explicit terms' vector-Jacobian product (k_vjp_combine's
// arithmetic) and the accumulation into the stage's cotangent in one pass.  out may be acc.
template <typename T>
__global__ __launch_bounds__(256) void k_vjp_close(const cx<T>* acc, const cx<T>* __restrict__ extra, const cx<T>* __restrict__ X,
                                                   size_t x_stride, const cx<T>* __restrict__ post, cx<T>* out, long total,
                                                   long plane) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long t = e % plane;
        cx<T> s = mk<T>((T)0, (T)0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const cx<T> x = X[(size_t)f * x_stride + e], q = post[(long)f * plane + t];
            s = s + mk<T>(x.x * q.x - x.y * q.y, x.x * q.y + x.y * q.x);
        }
        s = acc[e] + s;
        if (extra) s = s + extra[e];
        out[e] = s;
    }
}

// `steps` steps of the schedule of tcfd_ns2d_step_imex in reverse, last step first, for one chunk.  Per step: the stage states
// u_1 .. u_{nstages-1} are recomputed from the step's saved input (explicit_impl + k_stage_update, 4 launches per stage), then
// the stages are reversed: k_stage_adjoint, the adjoint sweep of the explicit terms at u_k (explicit_vjp_impl), k_vjp_close.
template <typename T, int N>
static int step_vjp_impl(const tcfd_ns2d_plan* p, const void* saved, size_t saved_step_stride, const void* g_out, const void* pre,
                         const void* post, void* g_in, long batch, int nstages, const double* fa, const double* beta,
                         const double* gdt, const double* mu, const double* mud, const int* base0, int steps, void* ws,
                         hipStream_t st) {
    VjpWs<T> V = carve_vjp<T>(p, ws, batch);
    const long plane = (long)N * p->m, total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    const T* lin = (const T*)p->lin;
    auto c = [&](const double* v, int k, double dflt) { return v ? (T)v[k] : (T)dflt; };
    const cx<T>* ub = (const cx<T>*)g_out;
    int rc;
    for (int s = steps - 1; s >= 0; --s) {
        const cx<T>* u0 = (const cx<T>*)saved + (size_t)s * saved_step_stride;
        auto state = [&](int k) { return k == 0 ? u0 : (const cx<T>*)(V.u + (size_t)(k - 1) * V.stride); };
        auto from_u0 = [&](int k) { return k > 0 && base0 && base0[k]; };    // (at k = 0 the initial state IS the current one)
        for (int k = 0; k + 1 < nstages; ++k) {
            if ((rc = explicit_impl<T, N>(p, state(k), V.F, nullptr, nullptr, false, batch, ws, st, 0))) return rc;
            hipLaunchKernelGGL(k_stage_update<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)V.F,
                               k ? (const cx<T>*)V.hf[(k - 1) & 1] : nullptr, from_u0(k) ? u0 : state(k), lin, c(fa, k, 1),
                               (T)beta[k], (T)gdt[k], (T)mu[k], c(mud, k, mu[k]), V.hf[k & 1],
                               V.u + (size_t)k * V.stride, total, plane);
            HIP_TRY(hipGetLastError());
        }
        bool ustart_live = false;
        for (int k = nstages - 1; k >= 0; --k) {
            hipLaunchKernelGGL(k_stage_adjoint<T>, dim3(blocks), dim3(256), 0, st, ub,
                               k == nstages - 1 ? nullptr : (const cx<T>*)V.hbar, lin, (const T*)pre, c(fa, k, 1), (T)beta[k],
                               (T)gdt[k], (T)mu[k], c(mud, k, mu[k]), V.gm, k ? V.hbar : nullptr, V.ubar,
                               from_u0(k) ? V.ustart : nullptr, ustart_live ? 1 : 0, total, plane);
            HIP_TRY(hipGetLastError());
            ustart_live |= from_u0(k);
            ub = V.ubar;
            if ((rc = explicit_vjp_impl<T, N>(p, state(k), V.gm, V.X, V.stride, batch, ws, st))) return rc;
            hipLaunchKernelGGL(k_vjp_close<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)V.ubar,
                               (k == 0 && ustart_live) ? (const cx<T>*)V.ustart : nullptr, (const cx<T>*)V.X, V.stride,
                               (const cx<T>*)post, (s == 0 && k == 0) ? (cx<T>*)g_in : V.ubar, total, plane);
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// ------------------------------------------------------------------ cotangent bundle: one trajectory, K cotangents
// The adjoint sweep of explicit_vjp_impl with the state's share done once: MODE_A on u_k (the caller: once per reversed stage),
// then group by group (kg cotangents, bundle_shape in tcfd_ns2d.hip) MODE_INV on the group's gm, ONE row pass for the group
// (k_rows_vjp_bundle, out of place: the state's planes serve every group), four MODE_FWD column transforms.  nbar is
// [cotangent][field] and Y [plane][cotangent][field], so the column passes are single launches over kn * batch fields wherever the
// arrays on both sides are tight; elsewhere they run per cotangent.  Sizes whose stash does not fit (bundle_two_pass, or
// TCFD_BUNDLE_ROWS = 0) run k_rows_vjp_oop once per cotangent: the state's planes are read again, nothing else of the state repeats.
template <typename T, int N>
static int launch_rows_vjp_bundle(const tcfd_ns2d_plan* p, const CoBundleWs<T>& W, int ncot, long batch, hipStream_t st) {
    const long npairs = batch * (N / 2);
    if (bundle_runs_two_pass<T, N>(p)) {
        constexpr int EPT = Cfg<T, N>::ROW_EPT, THR = Cfg<T, N>::ROW_THREADS;
        using Gm = RowGeom<T, N, EPT, THR>;
        auto kern = k_rows_vjp_oop<T, N, EPT, THR>;
        static DevOnce lds_once;
        if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
        const long blocks = rows_grid(p, (npairs + Gm::GROUPS - 1) / Gm::GROUPS, 4);
        for (int t = 0; t < ncot; ++t) {
            ProfScope prof(p, 1, st);
            hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const cx<T>*)W.planes, W.stride,
                               (const cx<T>*)(W.nbar + (size_t)t * W.stride), W.Y + (size_t)t * W.stride, W.yplane_stride,
                               (const cx<T>*)p->tw, npairs, p->ldw);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    }
    if constexpr (!bundle_two_pass<T, N>()) {
        constexpr int EPT = Cfg<T, N>::ROW_EPT;
        using Gm = BundleGeom<T, N, EPT>;
        auto kern = k_rows_vjp_bundle<T, N, EPT>;
        static DevOnce lds_once;
        if (int rc_ = set_lds(lds_once, kern, Gm::LDS_BYTES)) return rc_;
        const int per_cu = (int)std::min<size_t>(16, (160 * 1024) / Gm::LDS_BYTES);   // workgroups a CU holds
        const long blocks = rows_grid(p, (npairs + Gm::GROUPS - 1) / Gm::GROUPS, 2 * per_cu);
        // small problems: the cotangents are cut into segments until the device's workgroup slots are filled, as
        // launch_rows_jvp_bundle cuts the tangents; the bits do not depend on the cut
        const long slots = 256L * per_cu;
        const int segs = (int)std::max<long>(1, std::min<long>(ncot, slots / blocks));
        ProfScope prof(p, 1, st);
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)segs), dim3(Gm::THREADS), Gm::LDS_BYTES, st, (const cx<T>*)W.planes,
                           W.stride, (const cx<T>*)W.nbar, W.stride, W.Y, W.yplane_stride, W.stride, (const cx<T>*)p->tw, npairs,
                           p->ldw, ncot);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the opening column pass of the state of a reversed stage: u -> W.planes, once for every cotangent group
template <typename T, int N>
static int vjp_bundle_state(const tcfd_ns2d_plan* p, const CoBundleWs<T>& W, const cx<T>* u, long batch, hipStream_t st) {
    ColArgs<T> a{};
    a.planes = W.planes;
    a.plane_stride = W.stride;
    a.u_in = u;
    a.u_in_ld = p->m;
    a.nyq = 0;    // whole-column tiles, every column present (the row pass reads the plain layout)
    return launch_cols_v<T, N, MODE_A, Cfg<T, N>::COL_EPT, Cfg<T, N>::COLS>(p, a, batch, st);
}

// one group of kn cotangents through the sweep; gm: kn fields of batch, gm_ts apart (caller layout, pitch m);
// X_f of cotangent t -> xout + f * x_ps + t * x_ts (caller layout)
template <typename T, int N>
static int vjp_bundle_group(const tcfd_ns2d_plan* p, const CoBundleWs<T>& W, const cx<T>* gm, size_t gm_ts, cx<T>* xout, size_t x_ps,
                            size_t x_ts, long batch, int kn, hipStream_t st) {
    const size_t tight = (size_t)batch * N * p->m;                     // cotangents one after the other, caller layout
    const bool ws_tight = W.stride == (size_t)batch * N * p->ldw;     // a field's scratch is not padded
    int rc;
    ColArgs<T> g{};
    g.in_ld = p->m;
    g.out_ld = p->ldw;
    g.scale = (T)1;
    if (ws_tight && gm_ts == tight) {
        g.in = gm;
        g.out = W.nbar;
        if ((rc = launch_cols<T, N, MODE_INV>(p, g, (long)kn * batch, st))) return rc;
    } else {
        for (int t = 0; t < kn; ++t) {
            g.in = gm + (size_t)t * gm_ts;
            g.out = W.nbar + (size_t)t * W.stride;
            if ((rc = launch_cols<T, N, MODE_INV>(p, g, batch, st))) return rc;
        }
    }
    if ((rc = launch_rows_vjp_bundle<T, N>(p, W, kn, batch, st))) return rc;
    ColArgs<T> c{};
    c.in_ld = p->ldw;
    c.out_ld = p->m;
    c.scale = (T)1;
    for (int f = 0; f < 4; ++f) {
        if (ws_tight && x_ts == tight) {
            c.in = W.Y + (size_t)f * W.yplane_stride;
            c.out = xout + (size_t)f * x_ps;
            if ((rc = launch_cols<T, N, MODE_FWD>(p, c, (long)kn * batch, st))) return rc;
        } else {
            for (int t = 0; t < kn; ++t) {
                c.in = W.Y + (size_t)f * W.yplane_stride + (size_t)t * W.stride;
                c.out = xout + (size_t)f * x_ps + (size_t)t * x_ts;
                if ((rc = launch_cols<T, N, MODE_FWD>(p, c, batch, st))) return rc;
            }
        }
    }
    return 0;
}

template <typename T, int N>
static int explicit_vjp_bundle_impl(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, size_t cot_stride, long batch,
                                    int ncot, int kg, void* ws, hipStream_t st) {
    const CoBundleWs<T> W = carve_cobundle<T>(p, ws, batch, ncot, kg, 1);
    int rc;
    if ((rc = vjp_bundle_state<T, N>(p, W, (const cx<T>*)w, batch, st))) return rc;
    for (int k0 = 0; k0 < ncot; k0 += kg) {
        const int kn = std::min(kg, ncot - k0);
        if ((rc = vjp_bundle_group<T, N>(p, W, (const cx<T>*)gm + (size_t)k0 * cot_stride, cot_stride,
                                         (cx<T>*)xout + (size_t)k0 * 4 * cot_stride, cot_stride, 4 * cot_stride, batch, kn, st)))
            return rc;
    }
    return 0;
}

// k_stage_adjoint on K cotangents in one launch: the same arithmetic member by member (blockIdx.y strides over the members), one
// L and one `pre` table.  ub is `ub_ts` apart per member (the caller's g_out at the first reversed stage of a call, ubar after),
// every other array `ts`.  acc may be ub and hprev may be hb, as there -- no __restrict__ on them.
template <typename T>
struct StageAdjointBundleArgs {
    const cx<T>* ub; size_t ub_ts;
    const cx<T>* hb;
    const T* Lt; const T* pre;
    T fa, beta, gdt, mu, mud;
    cx<T>* gm; cx<T>* hprev; cx<T>* acc; cx<T>* ustart;
    int ustart_add;
    size_t ts;
    long total, plane;
    int ncot;
};
template <typename T>
__global__ __launch_bounds__(256) void k_stage_adjoint_bundle(StageAdjointBundleArgs<T> a) {
    for (int mem = blockIdx.y; mem < a.ncot; mem += gridDim.y) {
        const size_t o = (size_t)mem * a.ts;
        const cx<T>* ub = a.ub ? a.ub + (size_t)mem * a.ub_ts : nullptr;
        const cx<T>* hb = a.hb ? a.hb + o : nullptr;
        cx<T>* gm = a.gm + o;
        cx<T>* hprev = a.hprev ? a.hprev + o : nullptr;
        cx<T>* acc = a.acc + o;
        cx<T>* ustart = a.ustart ? a.ustart + o : nullptr;
        for (long e = blockIdx.x * 256L + threadIdx.x; e < a.total; e += (long)gridDim.x * 256L) {
            const long t = e % a.plane;
            const T L = a.Lt[t];
            cx<T> g = mk<T>((T)0, (T)0);
            if (ub) g = cscale(ub[e], fast_rcp((T)1 - a.mud * L));
            cx<T> G = cscale(g, a.gdt);
            if (hb) G = G + hb[e];
            gm[e] = cscale(cscale(G, a.fa), a.pre[t]);
            if (hprev) hprev[e] = cscale(G, a.beta);
            const cx<T> bb = g + cscale(cscale(g, L), a.mu);
            if (ustart) {
                ustart[e] = a.ustart_add ? ustart[e] + bb : bb;
                acc[e] = mk<T>((T)0, (T)0);
            } else {
                acc[e] = bb;
            }
        }
    }
}

// k_vjp_close on the members of one cotangent group in one launch: acc / extra `ts` apart per member, X `x_ts`, out `out_ts`
// (the caller's g_in at the last reversed stage of a call).  out may be acc.
template <typename T>
struct VjpCloseBundleArgs {
    const cx<T>* acc; const cx<T>* extra; size_t ts;
    const cx<T>* X; size_t x_stride, x_ts;
    const cx<T>* post;
    cx<T>* out; size_t out_ts;
    long total, plane;
    int ncot;
};
template <typename T>
__global__ __launch_bounds__(256) void k_vjp_close_bundle(VjpCloseBundleArgs<T> a) {
    for (int mem = blockIdx.y; mem < a.ncot; mem += gridDim.y) {
        const cx<T>* acc = a.acc + (size_t)mem * a.ts;
        const cx<T>* extra = a.extra ? a.extra + (size_t)mem * a.ts : nullptr;
        const cx<T>* X = a.X + (size_t)mem * a.x_ts;
        cx<T>* out = a.out + (size_t)mem * a.out_ts;
        for (long e = blockIdx.x * 256L + threadIdx.x; e < a.total; e += (long)gridDim.x * 256L) {
            const long t = e % a.plane;
            cx<T> s = mk<T>((T)0, (T)0);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const cx<T> x = X[(size_t)f * a.x_stride + e], q = a.post[(long)f * a.plane + t];
                s = s + mk<T>(x.x * q.x - x.y * q.y, x.x * q.y + x.y * q.x);
            }
            s = acc[e] + s;
            if (extra) s = s + extra[e];
            out[e] = s;
        }
    }
}

// step_vjp_impl for K cotangents of one trajectory: the stage states are recomputed ONCE per step, MODE_A runs ONCE per reversed
// stage, the element-wise kernels carry all K members, and the cotangents pass through the adjoint sweep group by group.
// g_out / g_in: K cotangents of batch fields, cot_stride apart.
template <typename T, int N>
static int step_vjp_bundle_impl(const tcfd_ns2d_plan* p, const void* saved, size_t saved_step_stride, const void* g_out,
                                const void* pre, const void* post, void* g_in, size_t cot_stride, long batch, int ncot, int kg,
                                int nstages, const double* fa, const double* beta, const double* gdt, const double* mu,
                                const double* mud, const int* base0, int steps, void* ws, hipStream_t st) {
    const CoBundleWs<T> V = carve_cobundle<T>(p, ws, batch, ncot, kg, nstages);
    const long plane = (long)N * p->m, total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    const T* lin = (const T*)p->lin;
    auto c = [&](const double* v, int k, double dflt) { return v ? (T)v[k] : (T)dflt; };
    cx<T>* F = V.planes;     // plane 0: free once the row pass of the recomputation has run
    const cx<T>* ub = (const cx<T>*)g_out;
    size_t ub_ts = cot_stride;
    int rc;
    for (int s = steps - 1; s >= 0; --s) {
        const cx<T>* u0 = (const cx<T>*)saved + (size_t)s * saved_step_stride;
        auto state = [&](int k) { return k == 0 ? u0 : (const cx<T>*)(V.u + (size_t)(k - 1) * V.stride); };
        auto from_u0 = [&](int k) { return k > 0 && base0 && base0[k]; };    // (at k = 0 the initial state IS the current one)
        for (int k = 0; k + 1 < nstages; ++k) {
            if ((rc = explicit_impl<T, N>(p, state(k), F, nullptr, nullptr, false, batch, ws, st, 0))) return rc;
            hipLaunchKernelGGL(k_stage_update<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)F,
                               k ? (const cx<T>*)V.hf[(k - 1) & 1] : nullptr, from_u0(k) ? u0 : state(k), lin, c(fa, k, 1),
                               (T)beta[k], (T)gdt[k], (T)mu[k], c(mud, k, mu[k]), V.hf[k & 1],
                               V.u + (size_t)k * V.stride, total, plane);
            HIP_TRY(hipGetLastError());
        }
        bool ustart_live = false;
        for (int k = nstages - 1; k >= 0; --k) {
            StageAdjointBundleArgs<T> a{};
            a.ub = ub; a.ub_ts = ub_ts;
            a.hb = k == nstages - 1 ? nullptr : (const cx<T>*)V.hbar;
            a.Lt = lin; a.pre = (const T*)pre;
            a.fa = c(fa, k, 1); a.beta = (T)beta[k]; a.gdt = (T)gdt[k]; a.mu = (T)mu[k]; a.mud = c(mud, k, mu[k]);
            a.gm = V.gm; a.hprev = k ? V.hbar : nullptr; a.acc = V.ubar;
            a.ustart = from_u0(k) ? V.ustart : nullptr; a.ustart_add = ustart_live ? 1 : 0;
            a.ts = V.tan_stride; a.total = total; a.plane = plane; a.ncot = ncot;
            hipLaunchKernelGGL(k_stage_adjoint_bundle<T>, dim3(blocks, (unsigned)std::min(ncot, 1024)), dim3(256), 0, st, a);
            HIP_TRY(hipGetLastError());
            ustart_live |= from_u0(k);
            ub = V.ubar;
            ub_ts = V.tan_stride;
            if ((rc = vjp_bundle_state<T, N>(p, V, state(k), batch, st))) return rc;
            const bool final = (s == 0 && k == 0);
            for (int k0 = 0; k0 < ncot; k0 += kg) {
                const int kn = std::min(kg, ncot - k0);
                if ((rc = vjp_bundle_group<T, N>(p, V, V.gm + (size_t)k0 * V.tan_stride, V.tan_stride, V.X, V.xplane_stride,
                                                 V.tan_stride, batch, kn, st)))
                    return rc;
                VjpCloseBundleArgs<T> cl{};
                cl.acc = V.ubar + (size_t)k0 * V.tan_stride;
                cl.extra = (k == 0 && ustart_live) ? V.ustart + (size_t)k0 * V.tan_stride : nullptr;
                cl.ts = V.tan_stride;
                cl.X = V.X; cl.x_stride = V.xplane_stride; cl.x_ts = V.tan_stride;
                cl.post = (const cx<T>*)post;
                cl.out = final ? (cx<T>*)g_in + (size_t)k0 * cot_stride : V.ubar + (size_t)k0 * V.tan_stride;
                cl.out_ts = final ? cot_stride : V.tan_stride;
                cl.total = total; cl.plane = plane; cl.ncot = kn;
                hipLaunchKernelGGL(k_vjp_close_bundle<T>, dim3(blocks, (unsigned)std::min(kn, 1024)), dim3(256), 0, st, cl);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return 0;
}

template <typename T, int N>
static int irfft2_sub_max_impl(const tcfd_ns2d_plan*) {
    using Gm = RowGeom<T, N, Cfg<T, N>::ROW_EPT>;
    return Gm::G < 64 ? Gm::G : 64;
}

template <typename T, int N>
static int variant_impl(const tcfd_ns2d_plan* p, int* split, int* rows_kernel) {
    const bool sp = use_split<T, N>(p);
    if (split) *split = sp ? 1 : 0;
    if (rows_kernel) {
        int v = p->tune.rows_v;
        if (v == 4 || v == 6) v = 5;                 // (removed kernels)
        if (v != 5 && v != 7) v = rows_default_version<T, N>();
        if (v == 7 && N != 1024) v = 5;
        *rows_kernel = v;
    }
    return 0;
}

// ------------------------------------------------------------------ the switch over n
// f(std::integral_constant<int, N>) for the plan's grid size
template <typename F>
static int by_size(int n, F&& f) {
    switch (n) {
#define TCFD_CASE(N) case N: return f(std::integral_constant<int, N>{});
        TCFD_NS2D_SIZES(TCFD_CASE)
#undef TCFD_CASE
        default: return fail(TCFD_EINVAL, "unsupported n=%d", n);
    }
}

namespace ns2d {
template <typename T>
int fill_round_fields(tcfd_ns2d_plan* p) {
    return by_size(p->n, [&](auto N) { return round_fields_impl<T, N()>(p); });
}
template <typename T>
int step(const tcfd_ns2d_plan* p, const void* w_in, void* w_out, void* dwdt, long batch, int nstages, const double* beta,
         const double* gdt, const double* mu_num, const double* fa, const double* mu_den, const int* base0, int steps,
         double inv_total_dt, void* ws, hipStream_t st, long ens_b0) {
    return by_size(p->n, [&](auto N) {
        return step_impl<T, N()>(p, w_in, w_out, dwdt, batch, nstages, beta, gdt, mu_num, fa, mu_den, base0, steps, inv_total_dt,
                                 ws, st, ens_b0);
    });
}
template <typename T>
int explicit_terms(const tcfd_ns2d_plan* p, const void* w, void* out, const void* wt, void* psi, bool residual, long batch,
                   void* ws, hipStream_t st, long ens_b0) {
    return by_size(p->n, [&](auto N) { return explicit_impl<T, N()>(p, w, out, wt, psi, residual, batch, ws, st, ens_b0); });
}
template <typename T>
int explicit_vjp(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, size_t x_field_stride, long batch, void* ws,
                 hipStream_t st) {
    return by_size(p->n, [&](auto N) { return explicit_vjp_impl<T, N()>(p, w, gm, xout, x_field_stride, batch, ws, st); });
}
template <typename T>
int explicit_jvp(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df, long batch, void* ws,
                 hipStream_t st) {
    return by_size(p->n, [&](auto N) { return explicit_jvp_impl<T, N()>(p, w, dw, out_f, out_df, batch, ws, st); });
}
template <typename T>
int step_jvp(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out, long batch, int nstages,
             const double* fa, const double* beta, const double* gdt, const double* mu_num, const double* mu_den,
             const int* base0, int steps, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) {
        return step_jvp_impl<T, N()>(p, w_in, dw_in, w_out, dw_out, batch, nstages, fa, beta, gdt, mu_num, mu_den, base0, steps,
                                     ws, st);
    });
}
template <typename T>
int explicit_jvp_bundle(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df, size_t tan_stride,
                        long batch, int ntan, int kg, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) {
        return explicit_jvp_bundle_entry<T, N()>(p, w, dw, out_f, out_df, tan_stride, batch, ntan, kg, ws, st);
    });
}
template <typename T>
int step_jvp_bundle(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out, size_t tan_stride,
                    long batch, int ntan, int kg, int nstages, const double* fa, const double* beta, const double* gdt,
                    const double* mu_num, const double* mu_den, const int* base0, int steps, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) {
        return step_jvp_bundle_impl<T, N()>(p, w_in, dw_in, w_out, dw_out, tan_stride, batch, ntan, kg, nstages, fa, beta, gdt,
                                            mu_num, mu_den, base0, steps, ws, st);
    });
}
template <typename T>
int step_vjp(const tcfd_ns2d_plan* p, const void* saved, size_t saved_step_stride, const void* g_out, const void* pre,
             const void* post, void* g_in, long batch, int nstages, const double* fa, const double* beta, const double* gdt,
             const double* mu_num, const double* mu_den, const int* base0, int steps, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) {
        return step_vjp_impl<T, N()>(p, saved, saved_step_stride, g_out, pre, post, g_in, batch, nstages, fa, beta, gdt, mu_num,
                                     mu_den, base0, steps, ws, st);
    });
}
template <typename T>
int explicit_vjp_bundle(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, size_t cot_stride, long batch, int ncot,
                        int kg, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) {
        return explicit_vjp_bundle_impl<T, N()>(p, w, gm, xout, cot_stride, batch, ncot, kg, ws, st);
    });
}
template <typename T>
int step_vjp_bundle(const tcfd_ns2d_plan* p, const void* saved, size_t saved_step_stride, const void* g_out, const void* pre,
                    const void* post, void* g_in, size_t cot_stride, long batch, int ncot, int kg, int nstages, const double* fa,
                    const double* beta, const double* gdt, const double* mu_num, const double* mu_den, const int* base0, int steps,
                    void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) {
        return step_vjp_bundle_impl<T, N()>(p, saved, saved_step_stride, g_out, pre, post, g_in, cot_stride, batch, ncot, kg, nstages,
                                            fa, beta, gdt, mu_num, mu_den, base0, steps, ws, st);
    });
}
template <typename T>
int rfft2(const tcfd_ns2d_plan* p, const void* x, void* out, long batch, hipStream_t st) {
    return by_size(p->n, [&](auto N) { return rfft2_impl<T, N()>(p, x, out, batch, st); });
}
template <typename T>
int irfft2(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) { return irfft2_impl<T, N()>(p, xh, out, batch, ws, st); });
}
template <typename T>
int irfft2_sub_max(const tcfd_ns2d_plan* p) {
    return by_size(p->n, [&](auto N) { return irfft2_sub_max_impl<T, N()>(p); });
}
template <typename T>
int irfft2_sub(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, int S, void* ws, hipStream_t st) {
    return by_size(p->n, [&](auto N) { return irfft2_sub_impl<T, N()>(p, xh, out, batch, S, ws, st); });
}
template <typename T>
int variant(const tcfd_ns2d_plan* p, int* split, int* rows_kernel) {
    return by_size(p->n, [&](auto N) { return variant_impl<T, N()>(p, split, rows_kernel); });
}

// explicit instantiation definitions for this unit's real type (the signatures are the declarations' in tcfd_ns2d_plan.hpp)
template decltype(fill_round_fields<TCFD_REAL>) fill_round_fields<TCFD_REAL>;
template decltype(step<TCFD_REAL>) step<TCFD_REAL>;
template decltype(explicit_terms<TCFD_REAL>) explicit_terms<TCFD_REAL>;
template decltype(explicit_vjp<TCFD_REAL>) explicit_vjp<TCFD_REAL>;
template decltype(explicit_jvp<TCFD_REAL>) explicit_jvp<TCFD_REAL>;
template decltype(step_jvp<TCFD_REAL>) step_jvp<TCFD_REAL>;
template decltype(explicit_jvp_bundle<TCFD_REAL>) explicit_jvp_bundle<TCFD_REAL>;
template decltype(step_jvp_bundle<TCFD_REAL>) step_jvp_bundle<TCFD_REAL>;
template decltype(step_vjp<TCFD_REAL>) step_vjp<TCFD_REAL>;
template decltype(explicit_vjp_bundle<TCFD_REAL>) explicit_vjp_bundle<TCFD_REAL>;
template decltype(step_vjp_bundle<TCFD_REAL>) step_vjp_bundle<TCFD_REAL>;
template decltype(rfft2<TCFD_REAL>) rfft2<TCFD_REAL>;
template decltype(irfft2<TCFD_REAL>) irfft2<TCFD_REAL>;
template decltype(irfft2_sub_max<TCFD_REAL>) irfft2_sub_max<TCFD_REAL>;
template decltype(irfft2_sub<TCFD_REAL>) irfft2_sub<TCFD_REAL>;
template decltype(variant<TCFD_REAL>) variant<TCFD_REAL>;
}  // namespace ns2d
