// tcfd_grf.hip -- MI355X (gfx950) kernel + C ABI of the Gaussian-random-field initial condition (reference:
// fno/data_gen/grf.py GRF2d.sample :79-115 and the "replicable init" of fno/data_gen/data_gen_fno.py:195-205).
//
// The reference draws complex noise c on an n0 x n0 mesh, takes s = Re(ifft2(E * c)) with the real table E = sqrt_eig,
// optionally keeps every (n0 / n)-th point, and the driver transforms the result with rfft2.  With V = E * c,
// H(k) = (V(k) + conj V(-k mod n0)) / 2 and st = n0 / n that chain is
//
//     rfft2(subsampled s)[kx, ky] = (n / n0)^2 * sum_{a, b < st} H(kx + a n, ky + b n),      kx < n, ky <= n / 2
//
// (the real part of an inverse transform keeps the Hermitian part of its spectrum; subsampling a mesh folds the aliases of
// its spectrum), so the half spectrum of a whole batch is one pass over the noise and no transform at all.
//
// Launch sequence:
//   k_grf_fold    one thread per output mode (kx, ky); the alias loop runs over (a, b), so for fixed (a, b) the lanes of a
//                 wave read adjacent ky: consecutive addresses at k, reversed-consecutive ones at -k.  Every noise element is
//                 read about once (columns 0 and n/2 of each alias class twice), the table once per sample.
//   k_grf_norm    (normalize only) one block per sample sums that sample's block partials in a fixed order
//   k_grf_scale   (normalize only) the spectrum times 1 / ||s / n0||_F
// The reference normalises on the n0 mesh BEFORE subsampling; by Parseval ||s||^2 = sum_k |H(k)|^2 / n0^2 over the full n0
// spectrum.  A thread visits the columns ky + b n with ky <= n / 2; the columns of the residues n - ky are the mirror images
// of those (|H(-k)| = |H(k)|), so every visited mode counts twice unless its residue is its own mirror (ky = 0, ky = n / 2).
// The partial sums are combined in a fixed order (wave shuffles, then the waves of a block, then the blocks of a sample):
// no floating-point atomics, two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tcfd_host.hpp"

// a * b - c * d must round both products: a contracted form leaves a residue where the two are equal, and the
// imaginary parts of the self-conjugate modes (and H(-k) = conj H(k) on the column ky = 0) are exact only without it
#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;   // 4 waves; 8 blocks per CU keep 32 waves of independent loads in flight

// sum over the block in a fixed order; the result is valid in thread 0
__device__ inline double block_sum(double v) {
    __shared__ double wave_sums[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBlock / 64; ++w) s += wave_sums[w];
    return s;
}

// noise[b][2][n0][n0] (plane 0 = Re c, plane 1 = Im c), eig[n0][n0], out[b][n][m] interleaved complex.
// partial[b][gridDim.x]: this block's share of sum_k |H(k)|^2 of sample b (normalize only, else null).
template <typename T>
__global__ void __launch_bounds__(kBlock) k_grf_fold(const T* __restrict__ noise, const T* __restrict__ eig,
                                                     T* __restrict__ out, double* __restrict__ partial, int n0, int n,
                                                     T fold_scale) {
    const int m = n / 2 + 1;
    const int st = n0 / n;
    const long plane = (long)n0 * n0;
    const long b = blockIdx.y;
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < (long)n * m;
    double sq = 0.0;
    if (live) {
        const int kx = (int)(t / m), ky = (int)(t % m);
        const T* __restrict__ re = noise + b * 2 * plane;
        const T* __restrict__ im = re + plane;
        T acc_re = 0, acc_im = 0;
        for (int a = 0; a < st; ++a) {
            const int r = kx + a * n;
            const int rn = r ? n0 - r : 0;
            for (int bb = 0; bb < st; ++bb) {
                const int c = ky + bb * n;
                const int cn = c ? n0 - c : 0;
                const long p = (long)r * n0 + c, q = (long)rn * n0 + cn;
                const T ep = eig[p], eq = eig[q];
                const T h_re = T(0.5) * (ep * re[p] + eq * re[q]);
                const T h_im = T(0.5) * (ep * im[p] - eq * im[q]);
                acc_re += h_re;
                acc_im += h_im;
                sq += (double)h_re * (double)h_re + (double)h_im * (double)h_im;
            }
        }
        T* o = out + 2 * (b * (long)n * m + t);
        o[0] = acc_re * fold_scale;
        o[1] = acc_im * fold_scale;
        if (ky != 0 && 2 * ky != n) sq *= 2.0;
    }
    if (partial != nullptr) {   // uniform over the grid
        const double s = block_sum(sq);
        if (threadIdx.x == 0) partial[b * gridDim.x + blockIdx.x] = s;
    }
}

// scale[b] = 1 / ||s / n0||_F = n0^2 / sqrt(sum_k |H(k)|^2); thread i adds partials i, i + 256, ... in that order
__global__ void __launch_bounds__(kBlock) k_grf_norm(const double* __restrict__ partial, double* __restrict__ scale, int nblocks,
                                                     double n0_sq) {
    const double* p = partial + (long)blockIdx.x * nblocks;
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kBlock) v += p[i];
    const double s = block_sum(v);
    if (threadIdx.x == 0) scale[blockIdx.x] = n0_sq / sqrt(s);
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_grf_scale(T* __restrict__ out, const double* __restrict__ scale, long per_sample) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= per_sample) return;
    const T s = (T)scale[blockIdx.y];
    out[blockIdx.y * per_sample + t] *= s;
}

inline long fold_blocks(int n) { return ((long)n * (n / 2 + 1) + kBlock - 1) / kBlock; }

template <typename T>
int run(const void* noise, const void* eig, void* out, long batch, int n0, int n, int normalize, void* workspace,
        hipStream_t stream) {
    const long nb = fold_blocks(n);
    double* partial = normalize ? static_cast<double*>(workspace) : nullptr;
    const double ratio = (double)n / (double)n0;
    const dim3 grid((unsigned)nb, (unsigned)batch);
    hipLaunchKernelGGL(k_grf_fold<T>, grid, dim3(kBlock), 0, stream, static_cast<const T*>(noise), static_cast<const T*>(eig),
                       static_cast<T*>(out), partial, n0, n, (T)(ratio * ratio));
    HIP_TRY(hipGetLastError());
    if (normalize) {
        double* scale = partial + batch * nb;
        hipLaunchKernelGGL(k_grf_norm, dim3((unsigned)batch), dim3(kBlock), 0, stream, partial, scale, (int)nb,
                           (double)n0 * (double)n0);
        HIP_TRY(hipGetLastError());
        const long per_sample = 2L * n * (n / 2 + 1);
        const dim3 sgrid((unsigned)((per_sample + kBlock - 1) / kBlock), (unsigned)batch);
        hipLaunchKernelGGL(k_grf_scale<T>, sgrid, dim3(kBlock), 0, stream, static_cast<T*>(out), scale, per_sample);
        HIP_TRY(hipGetLastError());
    }
    return TCFD_OK;
}

}  // namespace

extern "C" {

size_t tcfd_grf_spectrum_workspace_bytes(long batch, int n, int normalize) {
    if (!normalize || batch <= 0 || n <= 0) return 0;
    return (size_t)batch * (size_t)(fold_blocks(n) + 1) * sizeof(double);
}

int tcfd_grf_spectrum(const void* noise, const void* sqrt_eig, void* out, long batch, int n0, int n, int dtype, int normalize,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return FAIL(TCFD_EINVAL, "tcfd_grf_spectrum: dtype %d", dtype);
    if (n < 2 || n % 2 || n0 < n || n0 > 32768 || n0 % n)
        return FAIL(TCFD_EINVAL, "tcfd_grf_spectrum: n = %d must be even and divide n0 = %d (n0 <= 32768)", n, n0);
    if (batch < 0 || batch > 65535) return FAIL(TCFD_EINVAL, "tcfd_grf_spectrum: batch %ld outside 0 .. 65535", batch);
    if (batch == 0) return TCFD_OK;
    if (!noise || !sqrt_eig || !out) return FAIL(TCFD_EINVAL, "tcfd_grf_spectrum: null pointer");
    const size_t need = tcfd_grf_spectrum_workspace_bytes(batch, n, normalize);
    if (need && (!workspace || workspace_bytes < need))
        return FAIL(TCFD_EWORKSPACE, "tcfd_grf_spectrum: workspace %zu bytes, needs %zu", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == TCFD_C128 ? run<double>(noise, sqrt_eig, out, batch, n0, n, normalize, workspace, s)
                              : run<float>(noise, sqrt_eig, out, batch, n0, n, normalize, workspace, s);
}

}  // extern "C"
