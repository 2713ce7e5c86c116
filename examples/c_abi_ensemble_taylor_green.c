/* Per-sample physics through the C ABI alone (tcfd_ns2d_plan_set_ensemble): plain C99 against include/tcfd.h and the HIP runtime.
 *
 * Known-answer run: the Taylor-Green vortex  w0 = 2k cos(kx) cos(ky)  on [0, 2 pi)^2 decays like exp(-(2 nu k^2 + drag) t) under
 * viscosity nu and linear drag (the advection term vanishes).  ONE call steps three members with their own (nu, drag); each must
 * decay at its own analytic rate.  Then the program checks the contract around the mode: a batch that is not the member count is
 * refused naming both numbers, and count = 0 gives back the scalar plan.
 *
 *   gcc -std=c99 -O2 examples/c_abi_ensemble_taylor_green.c -Iinclude -I/opt/rocm/include -Ltorch-cfd_amd/csrc -L/opt/rocm/lib \
 *       -ltcfd_hip -lamdhip64 -lm -Wl,-rpath,$PWD/torch-cfd_amd/csrc -Wl,-rpath,/opt/rocm/lib -o c_abi_ensemble_taylor_green
 *   ./c_abi_ensemble_taylor_green      (tests/test_ns2d_ensemble_gpu.py::test_c_abi_ensemble_without_python builds and runs it)
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tcfd.h"

#define CHECK_HIP(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "HIP: %s\n", hipGetErrorString(e_)); return 2; } } while (0)
#define CHECK_TCFD(e) do { if ((e) != 0) { fprintf(stderr, "tcfd: %s\n", tcfd_last_error()); return 3; } } while (0)

#define MEMBERS 3

int main(void) {
    const int n = 64, m = n / 2 + 1, k = 2, steps = 100, batch = MEMBERS;
    const double PI = 3.14159265358979323846, L = 2 * PI, dt = 1e-2;
    const double nu[MEMBERS] = {1e-2, 3e-2, 1e-3}, drag[MEMBERS] = {0.0, 0.1, 0.5};
    double *kx = malloc(sizeof(double) * n), *ky = malloc(sizeof(double) * m);
    double *lap = malloc(sizeof(double) * n * m), *lin = malloc(sizeof(double) * n * m), *mask = calloc((size_t)n * m, sizeof(double));
    for (int i = 0; i < n; ++i) kx[i] = (i < n / 2 ? i : i - n) / L;        /* fftfreq(n, d = L / n) */
    for (int j = 0; j < m; ++j) ky[j] = (j < n / 2 ? j : j - n) / L;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            lap[i * m + j] = -4 * PI * PI * (kx[i] * kx[i] + ky[j] * ky[j]);
            lin[i * m + j] = nu[0] * lap[i * m + j] - drag[0];                 /* the plan's own table: member 0's */
        }
    {   /* 2/3-rule brick wall (see c_abi_taylor_green.c) */
        const int kr = (int)(2.0 / 3.0 * n), lo = kr / 2, hi = (kr + 1) / 2, cols = (int)(2.0 / 3.0 * m);
        for (int i = 0; i < n; ++i)
            if (i < lo || i >= n - hi)
                for (int j = 0; j < cols; ++j) mask[i * m + j] = 1.0;
    }
    tcfd_ns2d_plan* plan = NULL;
    CHECK_TCFD(tcfd_ns2d_plan_create(&plan, n, TCFD_C128, kx, ky, lin, mask, NULL));
    CHECK_TCFD(tcfd_ns2d_plan_set_ensemble(plan, batch, lap, nu, drag, NULL));   /* forcing_scale NULL: 1 (there is no forcing) */

    const size_t field = (size_t)n * m * 2, bytes = sizeof(double) * field * batch;
    double* h0 = calloc(field * batch, sizeof(double));
    for (int b = 0; b < batch; ++b) {
        const double amp = k * (double)n * n / 2;
        h0[b * field + ((size_t)k * m + k) * 2] = amp;
        h0[b * field + ((size_t)(n - k) * m + k) * 2] = amp;
    }
    void *w = NULL, *w_out = NULL, *ws = NULL;
    const size_t ws_bytes = tcfd_ns2d_workspace_bytes(plan, batch);
    CHECK_HIP(hipMalloc(&w, bytes));
    CHECK_HIP(hipMalloc(&w_out, bytes));
    CHECK_HIP(hipMalloc(&ws, ws_bytes));
    CHECK_HIP(hipMemcpy(w, h0, bytes, hipMemcpyHostToDevice));
    hipStream_t stream;
    CHECK_HIP(hipStreamCreate(&stream));

    const double alphas[6] = {0, 0.1496590219993, 0.3704009573644, 0.6222557631345, 0.9582821306748, 1};
    const double betas[5] = {0, -0.4178904745, -1.192151694643, -1.697784692471, -1.514183444257};
    const double gammas[5] = {0.1496590219993, 0.3792103129999, 0.8229550293869, 0.6994504559488, 0.1530572479681};
    double gdt[5], mu[5];
    for (int s = 0; s < 5; ++s) { gdt[s] = gammas[s] * dt; mu[s] = 0.5 * dt * (alphas[s + 1] - alphas[s]); }
    CHECK_TCFD(tcfd_ns2d_step(plan, w, w_out, NULL, batch, 5, betas, gdt, mu, steps, 1.0 / (steps * dt), ws, ws_bytes, (void*)stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    double* h1 = malloc(bytes);
    CHECK_HIP(hipMemcpy(h1, w_out, bytes, hipMemcpyDeviceToHost));

    int ok = 1;
    for (int b = 0; b < batch; ++b) {
        /* Crank-Nicolson is second order in dt: 100 steps of 1e-2 hold the analytic rate to ~1e-6 at the largest |L| dt here */
        const double decay = exp(-(2 * nu[b] * k * k + drag[b]) * dt * steps);
        double err2 = 0, ref2 = 0;
        for (size_t i = 0; i < field; ++i) {
            const double e = h1[b * field + i] - h0[b * field + i] * decay;
            err2 += e * e;
            ref2 += h0[b * field + i] * h0[b * field + i] * decay * decay;
        }
        const double rel = sqrt(err2 / ref2);
        printf("member %d: nu = %.0e, drag = %.1f: decay %.6f, rel-L2 error vs exp(-(2 nu k^2 + drag) t) = %.3e\n", b, nu[b], drag[b],
               decay, rel);
        if (!(rel < 1e-5)) ok = 0;
    }
    /* members differ: the wrong member's rate is far outside that bound */
    if (!(fabs(exp(-(2 * nu[0] * k * k + drag[0])) - exp(-(2 * nu[1] * k * k + drag[1]))) > 1e-2)) ok = 0;

    /* the contract: an ensemble plan steps exactly its members ... */
    int rc = tcfd_ns2d_step(plan, w, w_out, NULL, batch - 1, 5, betas, gdt, mu, 1, 1.0 / dt, ws, ws_bytes, (void*)stream);
    printf("batch %d on a %d-member plan: status %d (%s)\n", batch - 1, batch, rc, tcfd_last_error());
    if (rc != TCFD_EINVAL || !strstr(tcfd_last_error(), "batch 2") || !strstr(tcfd_last_error(), "3 fields")) ok = 0;
    /* ... and count = 0 gives back the scalar plan: every field at member 0's rate, any batch */
    CHECK_TCFD(tcfd_ns2d_plan_set_ensemble(plan, 0, NULL, NULL, NULL, NULL));
    CHECK_TCFD(tcfd_ns2d_step(plan, w, w_out, NULL, batch - 1, 5, betas, gdt, mu, steps, 1.0 / (steps * dt), ws, ws_bytes, (void*)stream));
    CHECK_HIP(hipStreamSynchronize(stream));
    CHECK_HIP(hipMemcpy(h1, w_out, bytes, hipMemcpyDeviceToHost));
    if (memcmp(h1, h1 + field, sizeof(double) * field) != 0) ok = 0;          /* fields 0 and 1: the same physics again */

    tcfd_ns2d_plan_destroy(plan);
    (void)hipFree(w); (void)hipFree(w_out); (void)hipFree(ws);
    if (!ok) { printf("FAIL\n"); return 1; }
    printf("PASS\n");
    return 0;
}
