// tcfd_loss_plan.hpp -- the plan of the loss kernels, shared by tcfd_loss.hip (which creates and destroys it) and
// tcfd_residual.hip (which reads its twiddle table)
#pragma once

struct tcfd_loss_plan {
    int n;       // square grid: 2^k in [16, 1024], 3 * 2^k in [96, 768] or 5 * 2^k in [80, 640]
    int dtype;   // TCFD_C64: float data, TCFD_C128: double data
    void* tw;    // [n] exp(-2 pi i k / n) in the plan's precision
};
