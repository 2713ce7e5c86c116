// tcfd_data.hip -- MI355X (gfx950) kernels + C ABI of the training data path: batches assembled from fields that stay on the
// device, and the Gaussian normalisers (reference: fno/datasets.py -- SpatioTemporalDataset.__getitem__ :431-453,
// SpatioTemporalDatasetFixedTime.__getitem__ :554-564, UnitGaussianNormalizer / SpatialGaussianNormalizer :21-121).
//
// The reference builds every sample on the CPU, stacks the samples and ships the batch; here a batch is one launch over
// the resident fields.  All four entry points only copy, cast and apply correctly rounded single operations, so their
// results equal the reference's bit for bit (the fitted statistics excepted: they are accumulated in fp64).
//
//   k_window        two adjacent time windows of listed samples at per-sample starts -> two time-last outputs.
//                   From time-first storage (N, T, P) this is a (steps, P) -> (P, steps) transposition per sample: a block
//                   takes 64 positions, its waves read whole time planes (64 consecutive elements per wave and plane),
//                   stage them through LDS rows of 64 + pad elements, and the block then stores ONE contiguous run of
//                   64 * steps elements.  pad is the inverse of steps mod 32 for odd steps (the 32 lanes of an LDS read
//                   group then hit 32 different banks), 1 for even steps.  From time-last storage (N, P, T) it is a
//                   gather of runs of `steps` elements, no staging.  grid.z = 0 / 1 selects the input / the output window.
//   k_fno3d_batch   plane c of sample s of the (b, 3 + steps, P, To) input: c < 3 a coordinate channel from the three host
//                   tables, else field plane c - 3 of row idx[s], every value repeated along the To output steps.  The
//                   planes b * (3 + steps) ... gather the target rows.  16-byte stores where a plane is a whole number
//                   of vectors; the (position, step) of each of a vector's elements is carried, not divided out again.
//   k_affine        (x - mean) / (std + eps)  and  x * (std + eps) + mean  with the statistic of element e at
//                   (e / inner) % m: inner = 1 is the trailing-shape broadcast of UnitGaussianNormalizer, inner = L the
//                   (..., 1) broadcast of SpatialGaussianNormalizer.  std + eps is rounded in the statistics' type, the
//                   rest in the promoted type, as torch does; a null mean is 0 (the backward of both forms).
//   k_moments_*     mean and unbiased std over axis 0 (cols: one thread column per statistic, 4 row groups combined in a
//                   fixed order) or over axis 0 and the last axis (rows: one block per statistic).  Two passes over the
//                   data inside one launch, fp64 accumulation in a fixed order, no atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "tcfd_host.hpp"

// x * s + m must round the product before the sum, as the two torch operations of the reference do
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;   // 4 waves
constexpr int kTile = 64;     // positions of one window tile: one wave reads one time plane of it per instruction
constexpr int kMaxSteps = 64; // steps of one window (LDS: 64 * (64 + 32) * 8 bytes = 48 KiB at most)

struct WindowArgs {
    const void* src;
    void* out[2];
    const long* idx;     // [count] rows of src
    const long* starts;  // [count] first step of the input window
    long rows, T, P;
    int steps[2];
    int pad[2];
    int time_last;
};

template <typename S, typename D>
__global__ void __launch_bounds__(kBlock) k_window(WindowArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    D* tile = reinterpret_cast<D*>(smem_raw);
    const int which = blockIdx.z;
    const int steps = a.steps[which];
    const long s = blockIdx.y;
    const long row = a.idx[s];
    const long t0 = a.starts[s] + (which ? a.steps[0] : 0);
    // the host has checked the lists; a block never leaves the source whatever they hold
    if (row < 0 || row >= a.rows || t0 < 0 || t0 + steps > a.T) return;
    const long p0 = (long)blockIdx.x * kTile;
    const int np = (int)((a.P - p0) < kTile ? (a.P - p0) : kTile);
    const S* __restrict__ src = static_cast<const S*>(a.src) + row * a.T * a.P;
    D* __restrict__ out = static_cast<D*>(a.out[which]) + (s * a.P + p0) * steps;
    const int run = np * steps;
    if (a.time_last) {
        const S* __restrict__ base = src + p0 * a.T + t0;
        for (int e = threadIdx.x; e < run; e += kBlock) {
            const int p = e / steps, t = e - p * steps;
            out[e] = (D)base[(long)p * a.T + t];
        }
        return;
    }
    const int stride = kTile + a.pad[which];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < np)
        for (int t = wave; t < steps; t += kBlock / 64) tile[t * stride + lane] = (D)src[(t0 + t) * a.P + p0 + lane];
    __syncthreads();
    for (int e = threadIdx.x; e < run; e += kBlock) {
        const int p = e / steps, t = e - p * steps;
        out[e] = tile[t * stride + p];
    }
}

struct Fno3dArgs {
    const void* field;   // (rows, steps, P)
    const void* target;  // (rows, P, To)
    const long* idx;     // [count]
    const void* gx;      // [n]  out dtype
    const void* gy;      // [n]
    const void* gt;      // [To]
    void* out_inp;       // (count, 3 + steps, P, To)
    void* out_tgt;       // (count, P, To)
    long rows, count;
    int steps, n, To;
};

template <typename S, typename D, int V>
__global__ void __launch_bounds__(kBlock) k_fno3d_batch(Fno3dArgs a) {
    const int C = 3 + a.steps;
    const long P = (long)a.n * a.n;
    const long plane = P * a.To;                       // elements of one output plane; a multiple of V
    const long e0 = ((long)blockIdx.x * kBlock + threadIdx.x) * V;
    if (e0 >= plane) return;
    const long y = blockIdx.y;
    D v[V];
    D* dst;
    if (y >= a.count * C) {                            // target rows
        const long s = y - a.count * C;
        const long row = a.idx[s];
        if (row < 0 || row >= a.rows) return;
        const S* __restrict__ src = static_cast<const S*>(a.target) + row * plane + e0;
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (D)src[j];
        dst = static_cast<D*>(a.out_tgt) + s * plane + e0;
    } else {
        const long s = y / C;
        const int c = (int)(y - s * C);
        const long row = a.idx[s];
        if (row < 0 || row >= a.rows) return;
        const unsigned To = (unsigned)a.To, n = (unsigned)a.n;   // a plane holds fewer than 2^31 elements (checked by the host)
        unsigned p = (unsigned)e0 / To;
        unsigned t = (unsigned)e0 - p * To;
        const S* __restrict__ f = static_cast<const S*>(a.field) + (row * a.steps + (c < 3 ? 0 : c - 3)) * P;
        const D* __restrict__ gx = static_cast<const D*>(a.gx);
        const D* __restrict__ gy = static_cast<const D*>(a.gy);
        const D* __restrict__ gt = static_cast<const D*>(a.gt);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            v[j] = c == 0 ? gx[p / n] : c == 1 ? gy[p % n] : c == 2 ? gt[t] : (D)f[p];
            if (++t == To) {
                t = 0;
                ++p;
            }
        }
        dst = static_cast<D*>(a.out_inp) + y * plane + e0;
    }
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (V == 2) {
        *reinterpret_cast<double2*>(dst) = make_double2(v[0], v[1]);
    } else {
        dst[0] = v[0];
    }
}

// out[e] = mode 0: (x[e] - mean[i]) / (std[i] + eps);  mode 1: x[e] * (std[i] + eps) + mean[i];  i = (e / inner) % m
template <typename X, typename S, typename O>
__global__ void __launch_bounds__(kBlock) k_affine(const X* __restrict__ x, const S* __restrict__ mean, const S* __restrict__ std_,
                                                   O* __restrict__ out, long total, long m, long inner, S eps, int mode) {
    using Pm = typename std::conditional<std::is_same<X, double>::value || std::is_same<S, double>::value, double, float>::type;
    const long stride = (long)gridDim.x * kBlock;
    const bool small = total <= 0x7fffffffL;   // 32-bit index arithmetic where it holds the element count
    for (long e = (long)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
        const long i = small ? (long)(((unsigned)e / (unsigned)inner) % (unsigned)m) : (e / inner) % m;
        const S se = std_[i] + eps;
        const Pm xv = (Pm)x[e];
        Pm r;
        if (mode == 0) {
            r = mean ? (xv - (Pm)mean[i]) / (Pm)se : xv / (Pm)se;
        } else {
            r = xv * (Pm)se;
            if (mean) r = r + (Pm)mean[i];
        }
        out[e] = (O)r;
    }
}

// x (rows, m): thread column c of a block owns statistic blockIdx.x * 64 + c; its 4 row groups take rows g, g + 4, ...
template <typename X, typename O>
__global__ void __launch_bounds__(kBlock) k_moments_cols(const X* __restrict__ x, O* __restrict__ mean, O* __restrict__ std_,
                                                         long rows, long m) {
    __shared__ double part[kBlock / 64][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long col = (long)blockIdx.x * 64 + c;
    const bool live = col < m;
    double acc = 0.0;
    if (live)
        for (long r = g; r < rows; r += kBlock / 64) acc += (double)x[r * m + col];
    part[g][c] = acc;
    __syncthreads();
    const double mu = (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) / (double)rows;
    __syncthreads();
    acc = 0.0;
    if (live)
        for (long r = g; r < rows; r += kBlock / 64) {
            const double d = (double)x[r * m + col] - mu;
            acc += d * d;
        }
    part[g][c] = acc;
    __syncthreads();
    if (live && g == 0) {
        const double ss = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
        mean[col] = (O)mu;
        std_[col] = (O)sqrt(ss / (double)(rows - 1));
    }
}

// sum over the block in a fixed order, returned to every thread
__device__ inline double block_sum_all(double v, double* wave_sums) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();   // wave_sums may still be read from the previous call
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

// x (rows, m, L): block i owns statistic i, reduced over the rows and the last axis
template <typename X, typename O>
__global__ void __launch_bounds__(kBlock) k_moments_rows(const X* __restrict__ x, O* __restrict__ mean, O* __restrict__ std_,
                                                         long rows, long m, long L) {
    __shared__ double wave_sums[kBlock / 64];
    const long i = blockIdx.x;
    const long count = rows * L;
    const X* __restrict__ base = x + i * L;
    double acc = 0.0;
    for (long j = threadIdx.x; j < count; j += kBlock) {
        const long r = j / L, l = j - r * L;
        acc += (double)base[r * m * L + l];
    }
    const double mu = block_sum_all(acc, wave_sums) / (double)count;
    acc = 0.0;
    for (long j = threadIdx.x; j < count; j += kBlock) {
        const long r = j / L, l = j - r * L;
        const double d = (double)base[r * m * L + l] - mu;
        acc += d * d;
    }
    const double ss = block_sum_all(acc, wave_sums);
    if (threadIdx.x == 0) {
        mean[i] = (O)mu;
        std_[i] = (O)sqrt(ss / (double)(count - 1));
    }
}

inline bool real_dtype(int d) { return d == TCFD_C64 || d == TCFD_C128; }

// pad of the LDS rows of a window of `steps` steps: the inverse of steps mod 32 for odd steps, else 1
inline int window_pad(int steps) {
    if (steps % 2 == 0) return 1;
    for (int c = 1; c < 32; c += 2)
        if ((c * steps) % 32 == 1) return c;
    return 1;
}

template <typename S, typename D>
int launch_window(const WindowArgs& a, long count, hipStream_t stream) {
    const int most = a.steps[0] > a.steps[1] ? a.steps[0] : a.steps[1];
    const size_t lds = a.time_last ? 0 : (size_t)most * (kTile + 32) * sizeof(D);
    const dim3 grid((unsigned)((a.P + kTile - 1) / kTile), (unsigned)count, 2);
    hipLaunchKernelGGL((k_window<S, D>), grid, dim3(kBlock), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return TCFD_OK;
}

template <typename S, typename D>
int launch_fno3d(const Fno3dArgs& a, hipStream_t stream) {
    constexpr int VW = 16 / sizeof(D);
    const long plane = (long)a.n * a.n * a.To;
    const long planes = a.count * (3 + a.steps) + a.count;
    if (plane % VW == 0) {
        const dim3 grid((unsigned)((plane / VW + kBlock - 1) / kBlock), (unsigned)planes);
        hipLaunchKernelGGL((k_fno3d_batch<S, D, VW>), grid, dim3(kBlock), 0, stream, a);
    } else {
        const dim3 grid((unsigned)((plane + kBlock - 1) / kBlock), (unsigned)planes);
        hipLaunchKernelGGL((k_fno3d_batch<S, D, 1>), grid, dim3(kBlock), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return TCFD_OK;
}

template <typename X, typename S, typename O>
int launch_affine(const void* x, const void* mean, const void* std_, void* out, long total, long m, long inner, double eps,
                  int mode, hipStream_t stream) {
    long blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 256L * 32) blocks = 256L * 32;   // grid-stride beyond 32 blocks per CU
    hipLaunchKernelGGL((k_affine<X, S, O>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, static_cast<const X*>(x),
                       static_cast<const S*>(mean), static_cast<const S*>(std_), static_cast<O*>(out), total, m, inner, (S)eps,
                       mode);
    HIP_TRY(hipGetLastError());
    return TCFD_OK;
}

template <typename X, typename O>
int launch_moments(const void* x, void* mean, void* std_, long rows, long m, long L, hipStream_t stream) {
    if (L == 1) {
        hipLaunchKernelGGL((k_moments_cols<X, O>), dim3((unsigned)((m + 63) / 64)), dim3(kBlock), 0, stream,
                           static_cast<const X*>(x), static_cast<O*>(mean), static_cast<O*>(std_), rows, m);
    } else {
        hipLaunchKernelGGL((k_moments_rows<X, O>), dim3((unsigned)m), dim3(kBlock), 0, stream, static_cast<const X*>(x),
                           static_cast<O*>(mean), static_cast<O*>(std_), rows, m, L);
    }
    HIP_TRY(hipGetLastError());
    return TCFD_OK;
}

}  // namespace

extern "C" {

int tcfd_data_window(const void* src, void* out_in, void* out_out, const void* idx, const void* starts, long count, long rows,
                     long total_steps, long points, int steps, int out_steps, int time_last, int src_dtype, int dst_dtype,
                     void* stream) {
    if (!real_dtype(src_dtype) || !real_dtype(dst_dtype))
        return FAIL(TCFD_EINVAL, "tcfd_data_window: dtypes %d -> %d", src_dtype, dst_dtype);
    if (steps < 1 || out_steps < 1 || steps > kMaxSteps || out_steps > kMaxSteps)
        return FAIL(TCFD_EINVAL, "tcfd_data_window: steps %d, out_steps %d outside 1 .. %d", steps, out_steps, kMaxSteps);
    if (rows < 1 || points < 1 || total_steps < (long)steps + out_steps)
        return FAIL(TCFD_EINVAL, "tcfd_data_window: source (%ld, %ld, %ld) holds no window of %d + %d steps", rows, total_steps,
                    points, steps, out_steps);
    if (count < 0 || count > 65535) return FAIL(TCFD_EINVAL, "tcfd_data_window: count %ld outside 0 .. 65535", count);
    if ((points + kTile - 1) / kTile > 0x7fffffffL) return FAIL(TCFD_EINVAL, "tcfd_data_window: %ld points", points);
    if (count == 0) return TCFD_OK;
    if (!src || !out_in || !out_out || !idx || !starts) return FAIL(TCFD_EINVAL, "tcfd_data_window: null pointer");
    WindowArgs a;
    a.src = src;
    a.out[0] = out_in;
    a.out[1] = out_out;
    a.idx = static_cast<const long*>(idx);
    a.starts = static_cast<const long*>(starts);
    a.rows = rows;
    a.T = total_steps;
    a.P = points;
    a.steps[0] = steps;
    a.steps[1] = out_steps;
    a.pad[0] = window_pad(steps);
    a.pad[1] = window_pad(out_steps);
    a.time_last = time_last != 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (src_dtype == TCFD_C64)
        return dst_dtype == TCFD_C64 ? launch_window<float, float>(a, count, s) : launch_window<float, double>(a, count, s);
    return dst_dtype == TCFD_C64 ? launch_window<double, float>(a, count, s) : launch_window<double, double>(a, count, s);
}

int tcfd_data_fno3d_batch(const void* field, const void* target, const void* idx, const void* grid_x, const void* grid_y,
                          const void* grid_t, void* out_input, void* out_target, long count, long rows, int steps, int n,
                          int out_steps, int src_dtype, int dst_dtype, void* stream) {
    if (!real_dtype(src_dtype) || !real_dtype(dst_dtype))
        return FAIL(TCFD_EINVAL, "tcfd_data_fno3d_batch: dtypes %d -> %d", src_dtype, dst_dtype);
    if (steps < 1 || n < 1 || out_steps < 1 || n > 32768 || rows < 1)
        return FAIL(TCFD_EINVAL, "tcfd_data_fno3d_batch: steps %d, n %d, out_steps %d, rows %ld", steps, n, out_steps, rows);
    if ((long)n * n * out_steps > 0x7fffffffL)
        return FAIL(TCFD_EINVAL, "tcfd_data_fno3d_batch: a plane of %d x %d x %d elements exceeds 2^31 - 1", n, n, out_steps);
    if (count < 0 || count * (4 + (long)steps) > 65535)
        return FAIL(TCFD_EINVAL, "tcfd_data_fno3d_batch: count %ld: count * (4 + steps) may not exceed 65535", count);
    if (count == 0) return TCFD_OK;
    if (!field || !target || !idx || !grid_x || !grid_y || !grid_t || !out_input || !out_target)
        return FAIL(TCFD_EINVAL, "tcfd_data_fno3d_batch: null pointer");
    Fno3dArgs a;
    a.field = field;
    a.target = target;
    a.idx = static_cast<const long*>(idx);
    a.gx = grid_x;
    a.gy = grid_y;
    a.gt = grid_t;
    a.out_inp = out_input;
    a.out_tgt = out_target;
    a.rows = rows;
    a.count = count;
    a.steps = steps;
    a.n = n;
    a.To = out_steps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (src_dtype == TCFD_C64) return dst_dtype == TCFD_C64 ? launch_fno3d<float, float>(a, s) : launch_fno3d<float, double>(a, s);
    return dst_dtype == TCFD_C64 ? launch_fno3d<double, float>(a, s) : launch_fno3d<double, double>(a, s);
}

int tcfd_data_affine(const void* x, const void* mean, const void* std_, void* out, long total, long stat_count, long inner,
                     double eps, int mode, int x_dtype, int stat_dtype, int out_dtype, void* stream) {
    if (!real_dtype(x_dtype) || !real_dtype(stat_dtype) || !real_dtype(out_dtype))
        return FAIL(TCFD_EINVAL, "tcfd_data_affine: dtypes %d, %d -> %d", x_dtype, stat_dtype, out_dtype);
    if (mode != 0 && mode != 1) return FAIL(TCFD_EINVAL, "tcfd_data_affine: mode %d", mode);
    if (total < 0 || stat_count < 1 || inner < 1 || total % (stat_count * inner))
        return FAIL(TCFD_EINVAL, "tcfd_data_affine: %ld elements are no multiple of %ld statistics x %ld", total, stat_count, inner);
    if (total == 0) return TCFD_OK;
    if (!x || !std_ || !out) return FAIL(TCFD_EINVAL, "tcfd_data_affine: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int key = (x_dtype == TCFD_C128) * 4 + (stat_dtype == TCFD_C128) * 2 + (out_dtype == TCFD_C128);
#define AFFINE(X, S, O) return launch_affine<X, S, O>(x, mean, std_, out, total, stat_count, inner, eps, mode, s)
    switch (key) {
        case 0: AFFINE(float, float, float);
        case 1: AFFINE(float, float, double);
        case 2: AFFINE(float, double, float);
        case 3: AFFINE(float, double, double);
        case 4: AFFINE(double, float, float);
        case 5: AFFINE(double, float, double);
        case 6: AFFINE(double, double, float);
        default: AFFINE(double, double, double);
    }
#undef AFFINE
}

int tcfd_data_moments(const void* x, void* mean, void* std_, long rows, long stat_count, long inner, int x_dtype, int stat_dtype,
                      void* stream) {
    if (!real_dtype(x_dtype) || !real_dtype(stat_dtype))
        return FAIL(TCFD_EINVAL, "tcfd_data_moments: dtypes %d -> %d", x_dtype, stat_dtype);
    if (rows < 1 || stat_count < 1 || inner < 1 || stat_count > 0x7fffffffL)
        return FAIL(TCFD_EINVAL, "tcfd_data_moments: shape (%ld, %ld, %ld)", rows, stat_count, inner);
    if (!x || !mean || !std_) return FAIL(TCFD_EINVAL, "tcfd_data_moments: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (x_dtype == TCFD_C64)
        return stat_dtype == TCFD_C64 ? launch_moments<float, float>(x, mean, std_, rows, stat_count, inner, s)
                                      : launch_moments<float, double>(x, mean, std_, rows, stat_count, inner, s);
    return stat_dtype == TCFD_C64 ? launch_moments<double, float>(x, mean, std_, rows, stat_count, inner, s)
                                  : launch_moments<double, double>(x, mean, std_, rows, stat_count, inner, s);
}

}  // extern "C"
