// tcfd_loss_plan.hpp -- what tcfd_loss.hip and tcfd_residual.hip share: the plan of the loss kernels (tcfd_loss.hip creates
// and destroys it, tcfd_residual.hip reads its twiddle table) and the host helper that raises a kernel's dynamic-LDS limit
#pragma once
#include <atomic>

#include "tcfd_host.hpp"

struct tcfd_loss_plan {
    int n;       // square grid: 2^k in [16, 1024], 3 * 2^k in [96, 768] or 5 * 2^k in [80, 640]
    int dtype;   // TCFD_C64: float data, TCFD_C128: double data
    void* tw;    // [n] exp(-2 pi i k / n) in the plan's precision
};

// the dynamic-LDS attribute of a kernel is set once per (kernel instantiation, device)
template <typename K>
static int raise_lds(K kernel, size_t bytes) {
    static std::atomic<unsigned long long> done{0};     // one per instantiation of this template = per kernel
    if (bytes <= 48 * 1024) return 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}
