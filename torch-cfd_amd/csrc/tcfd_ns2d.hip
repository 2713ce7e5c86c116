// tcfd_ns2d.hip -- the C ABI of the batched 2-D pseudo-spectral vorticity solver (include/tcfd.h, tcfd_ns2d_adjoint.h): the library's error state,
// plans, argument checks and batch chunking, and the kernels that do not depend on the grid size.  The size-templated kernels
// live in tcfd_ns2d_sized.hip, built once per precision; an entry point here checks its arguments, cuts the batch into chunks
// and calls the sized unit of the plan's precision through the ns2d:: templates of tcfd_ns2d_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <unistd.h>
#include <limits>
#include <vector>

#include "tcfd_ns2d_plan.hpp"
#include "../../include/tcfd_ns2d_adjoint.h"
#include "../../include/tcfd_ns2d_bundle.h"
#include "../../include/tcfd_ns2d_adjoint_bundle.h"

using namespace tcfd;

// op<double> or op<float> of the sized units, by the plan's precision
#define NS2D_SIZED(p, op, ...) \
    ((p)->dtype == TCFD_C128 ? ns2d::op<double>(__VA_ARGS__) : ns2d::op<float>(__VA_ARGS__))

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int tcfd_set_error(int code, const char* fmt, ...) {  // shared by every unit of the library (tcfd_host.hpp)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* tcfd_last_error(void) { return g_err; }
extern "C" int tcfd_version(void) { return TCFD_ABI_VERSION; }

// ------------------------------------------------------------------ plan
static bool supported_n(int n) {
#define TCFD_IS_N(N) || n == N
    return false TCFD_NS2D_SIZES(TCFD_IS_N);
#undef TCFD_IS_N
}

template <typename T>
static int upload(void** dst, const std::vector<T>& host) {
    HIP_TRY(hipMalloc(dst, host.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

template <typename T>
static int plan_fill(tcfd_ns2d_plan* p, const double* kx, const double* ky, const double* lin, const double* mask,
                     const double* forcing) {
    const int n = p->n, m = p->m;
    std::vector<T> tw(2 * (size_t)n), a(n), b(m), l((size_t)n * m), k((size_t)n * m);
    for (int t = 0; t < n; ++t) {
        // long-double evaluation, rounded once to the working type
        const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)t / (long double)n;
        tw[2 * t] = (T)cosl(ang);
        tw[2 * t + 1] = (T)sinl(ang);
    }
    // exact values at the quadrant points
    tw[0] = 1; tw[1] = 0;
    tw[2 * (n / 4)] = 0; tw[2 * (n / 4) + 1] = -1;
    tw[2 * (n / 2)] = -1; tw[2 * (n / 2) + 1] = 0;
    tw[2 * (3 * n / 4)] = 0; tw[2 * (3 * n / 4) + 1] = 1;
    for (int i = 0; i < n; ++i) a[i] = (T)kx[i];
    for (int i = 0; i < m; ++i) b[i] = (T)ky[i];
    for (size_t i = 0; i < (size_t)n * m; ++i) { l[i] = (T)lin[i]; k[i] = (T)mask[i]; }
    int rc;
    if ((rc = upload(&p->tw, tw))) return rc;
    {
        std::vector<T> t2((size_t)n);  // W_{n/2}^t = W_n^{2t}
        for (int t = 0; t < n / 2; ++t) { t2[2 * t] = tw[2 * (2 * t)]; t2[2 * t + 1] = tw[2 * (2 * t) + 1]; }
        if ((rc = upload(&p->tw2, t2))) return rc;
    }
    if ((rc = upload(&p->kx, a))) return rc;
    if ((rc = upload(&p->ky, b))) return rc;
    if ((rc = upload(&p->lin, l))) return rc;
    if ((rc = upload(&p->mask, k))) return rc;
    const bool force_tables = env_int("TCFD_FORCE_TABLES", 0) != 0;
    // --- separable forms: mask = r[i]*c[j] (exact for 0/1 brick walls), lin = a[i] + b[j]
    {
        std::vector<T> mr(n, 0), mc(m, 0), lr(n), lc(m);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) {
                mr[i] = std::max(mr[i], k[(size_t)i * m + j]);
                mc[j] = std::max(mc[j], k[(size_t)i * m + j]);
            }
        bool ok = true;
        T lmax = 0;
        for (int j = 0; j < m; ++j) lc[j] = l[j];
        for (int i = 0; i < n; ++i) lr[i] = l[(size_t)i * m] - l[0];
        for (size_t i = 0; i < (size_t)n * m; ++i) lmax = std::max(lmax, (T)std::fabs(l[i]));
        const T tol = (T)8 * std::numeric_limits<T>::epsilon() * lmax;
        for (int i = 0; i < n && ok; ++i)
            for (int j = 0; j < m; ++j) {
                if (k[(size_t)i * m + j] != mr[i] * mc[j]) { ok = false; break; }
                if (std::fabs(l[(size_t)i * m + j] - (lr[i] + lc[j])) > tol) { ok = false; break; }
            }
        p->sep = (ok && !force_tables) ? 1 : 0;
        // prunable: mask_c is a 1...1 0...0 prefix pattern and every forcing entry sits where the mask is 1
        int kc = 0;
        while (kc < m && mc[kc] == (T)1) ++kc;
        bool prefix = p->sep && kc < m;
        for (int j = kc; j < m && prefix; ++j) prefix = (mc[j] == (T)0);
        for (int i = 0; i < n && prefix; ++i) prefix = (mr[i] == (T)0 || mr[i] == (T)1);
        if (prefix && forcing)
            for (size_t e = 0; e < (size_t)n * m && prefix; ++e)
                if ((forcing[2 * e] != 0 || forcing[2 * e + 1] != 0) && k[e] == (T)0) prefix = false;
        p->keep_cols = (prefix && !env_int("TCFD_NO_PRUNE", 0)) ? kc : 0;
        if (p->sep) {
            if ((rc = upload(&p->mask_r, mr))) return rc;
            if ((rc = upload(&p->mask_c, mc))) return rc;
            if ((rc = upload(&p->lin_r, lr))) return rc;
            if ((rc = upload(&p->lin_c, lc))) return rc;
        }
    }
    if (forcing) {
        std::vector<T> f(2 * (size_t)n * m);
        for (size_t i = 0; i < f.size(); ++i) f[i] = (T)forcing[i];
        size_t nnz = 0;
        for (size_t i = 0; i < (size_t)n * m; ++i) nnz += (f[2 * i] != 0 || f[2 * i + 1] != 0);
        if (nnz * 64 <= (size_t)n * m && !force_tables) {  // sparse: column-compressed list
            std::vector<int> ptr(m + 1, 0), row, col;
            std::vector<T> val;
            for (int j = 0; j < m; ++j) {
                for (int i = 0; i < n; ++i) {
                    const size_t e = (size_t)i * m + j;
                    if (f[2 * e] != 0 || f[2 * e + 1] != 0) {
                        row.push_back(i);
                        col.push_back(j);
                        val.push_back(f[2 * e]);
                        val.push_back(f[2 * e + 1]);
                    }
                }
                ptr[j + 1] = (int)row.size();
            }
            p->f_nnz = (int)row.size();
            if (row.empty()) { row.push_back(0); col.push_back(0); val.push_back(0); val.push_back(0); }
            p->f_sparse = 1;
            if ((rc = upload(&p->f_col, col))) return rc;
            if ((rc = upload(&p->f_ptr, ptr))) return rc;
            if ((rc = upload(&p->f_row, row))) return rc;
            if ((rc = upload(&p->f_val, val))) return rc;
        } else if ((rc = upload(&p->forcing, f))) {
            return rc;
        }
    }
    return 0;
}

extern "C" void tcfd_ns2d_plan_destroy(tcfd_ns2d_plan* p) {
    if (!p) return;
    void* ptrs[] = {p->tw, p->tw2, p->kx, p->ky, p->lin, p->mask, p->forcing, p->mask_r, p->mask_c,
                    p->lin_r, p->lin_c, p->f_ptr, p->f_row, p->f_val, p->f_col, p->ens, p->lap, p->lap_r, p->lap_c};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    if (p->prof) {
        for (auto& r : p->prof->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        delete p->prof;
    }
    if (p->gs) {
        if (p->gs->exec) (void)hipGraphExecDestroy(p->gs->exec);
        if (p->gs->graph) (void)hipGraphDestroy(p->gs->graph);
        if (p->gs->exec_multi) (void)hipGraphExecDestroy(p->gs->exec_multi);
        if (p->gs->graph_multi) (void)hipGraphDestroy(p->gs->graph_multi);
        if (p->gs->ev_in) (void)hipEventDestroy(p->gs->ev_in);
        if (p->gs->ev_out) (void)hipEventDestroy(p->gs->ev_out);
        if (p->gs->ev_out2) (void)hipEventDestroy(p->gs->ev_out2);
        if (p->gs->ev_rows) (void)hipEventDestroy(p->gs->ev_rows);
        if (p->gs->stream2) (void)hipStreamDestroy(p->gs->stream2);
        if (p->gs->stream) (void)hipStreamDestroy(p->gs->stream);
        delete p->gs;
    }
    delete p;
}

// Size of the memory-side last-level cache (Infinity Cache / MALL) of the CURRENT device.  hipDeviceProp_t has no field
// for it (l2CacheSize is the per-XCD L2); the KFD topology does: the level-3 entry under
// /sys/class/kfd/kfd/topology/nodes/<node>/caches/, the node matched to the device by PCI location.  TCFD_CACHE_MB
// overrides; 256 MB (MI355X) when the topology cannot be read.
static size_t last_level_cache_bytes(int* source) {
    *source = 0;
    const int forced = env_int("TCFD_CACHE_MB", 0);
    if (forced > 0) { *source = 2; return (size_t)forced << 20; }
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return (size_t)256 << 20;
    const long want_loc = ((long)prop.pciBusID << 8) | ((long)prop.pciDeviceID << 3);
    auto read_props = [](const char* path, const char* const* keys, long* vals, int nk) {
        FILE* f = fopen(path, "r");
        if (!f) return false;
        char key[128];
        long long v;
        while (fscanf(f, "%127s %lld", key, &v) == 2)
            for (int i = 0; i < nk; ++i)
                if (!strcmp(key, keys[i])) vals[i] = (long)v;
        fclose(f);
        return true;
    };
    // Pass 1: the node whose PCI location is this device's.  Pass 2 (containers hide the GPU nodes' `properties` files but not
    // their cache entries): every node that lists a level-3 cache -- the GPUs of one box are of one kind, so the smallest
    // level-3 size found is this device's (and the safe choice if they were not).
    long any_l3 = 0;
    for (int node = 0; node < 128; ++node) {
        char path[256];
        snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/properties", node);
        const char* nkeys[] = {"simd_count", "location_id", "domain"};
        long nv[3] = {-1, -1, 0};
        const bool props = read_props(path, nkeys, nv, 3);
        snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/caches", node);
        if (!props && access(path, F_OK) != 0) { if (node > 16) break; else continue; }
        if (props && nv[0] == 0) continue;       // a CPU node
        long best = 0;
        for (int c = 0; c < 1024; ++c) {
            snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/caches/%d/properties", node, c);
            const char* ckeys[] = {"level", "size"};
            long cv[2] = {0, 0};
            if (!read_props(path, ckeys, cv, 2)) break;
            if (cv[0] >= 3 && cv[1] > best) best = cv[1];   // size is in KB
        }
        if (best <= 0) continue;
        if (props && nv[1] == want_loc && nv[2] == (long)prop.pciDomainID) { *source = 1; return (size_t)best << 10; }
        if (any_l3 == 0 || best < any_l3) any_l3 = best;
    }
    if (any_l3 > 0) { *source = 1; return (size_t)any_l3 << 10; }
    return (size_t)256 << 20;
}

extern "C" int tcfd_ns2d_plan_create(tcfd_ns2d_plan** out, int n, int dtype, const double* kx, const double* ky,
                                     const double* linear_term, const double* mask, const double* forcing_hat) {
    if (!out || !kx || !ky || !linear_term || !mask) return fail(TCFD_EINVAL, "plan_create: null argument");
    if (!supported_n(n)) return fail(TCFD_EINVAL, "plan_create: n=%d is not a power of two in [8, 4096] (or 3 * 2^k in 96..1536, 5 * 2^k in 80..1280)", n);
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return fail(TCFD_EINVAL, "plan_create: bad dtype %d", dtype);
    tcfd_ns2d_plan* p = new tcfd_ns2d_plan();   // value-initialised: every pointer / flag starts at zero
    p->n = n;
    p->m = n / 2 + 1;
    p->dtype = dtype;
    p->tune.split = env_int("TCFD_SPLIT", -1);
    p->tune.small_tiles = env_int("TCFD_SMALL_TILES", -1);
    p->tune.two_wg = env_int("TCFD_TWO_WG", 1);
    p->tune.f32_cols8 = env_int("TCFD_F32_COLS8", 1);
    p->tune.rows7_minw = env_int("TCFD_ROWS7_MINW", 4);
    p->tune.cols_lds_pad = env_int("TCFD_COLS_LDS_PAD", 0);
    p->tune.nt_out = env_int("TCFD_NT_OUT", 0);
    p->tune.rows_blocks_per_cu = env_int("TCFD_ROWS_BLOCKS_PER_CU", 0);
    p->tune.pair_xcd = env_int("TCFD_PAIR_XCD", 1);
    p->tune.ablate = env_int("TCFD_ABLATE", 0);
    p->tune.nt_planes = env_int("TCFD_NT_PLANES", -1);
    p->tune.rows_v = env_int("TCFD_ROWS_V", 0);
    p->tune.chunk = env_int("TCFD_CHUNK", -1);
    p->tune.bundle_rows = env_int("TCFD_BUNDLE_ROWS", -1);
    p->tune.cols_xl = env_int("TCFD_COLS_XL", 1);
    p->tune.nyq_pack = env_int("TCFD_NYQ_PACK", 1);
    p->tune.graph = env_int("TCFD_GRAPH", -1);
    p->tune.overlap = env_int("TCFD_OVERLAP", 0);
    p->tune.cache_bytes = last_level_cache_bytes(&p->tune.cache_source);
    {
        const int per_line = dtype == TCFD_C128 ? 8 : 16;  // complex elements per 128-byte line
        p->ldw = (p->m + per_line - 1) / per_line * per_line;
    }
    int rc = dtype == TCFD_C128 ? plan_fill<double>(p, kx, ky, linear_term, mask, forcing_hat)
                                : plan_fill<float>(p, kx, ky, linear_term, mask, forcing_hat);
    if (rc) {
        tcfd_ns2d_plan_destroy(p);
        return rc;
    }
    (void)NS2D_SIZED(p, fill_round_fields, p);   // (needs the size switch)
    // (one-column tiles -- 4096^2 fp64 with TCFD_SPLIT=0 -- cannot pack: tile 0 builds Z in TWO columns' worth of exchange buffer)
    const bool one_column_tiles = n == 4096 && dtype == TCFD_C128 && p->tune.split == 0;
    p->nyq = (p->tune.nyq_pack && n >= 64 && (n & (n - 1)) == 0 && p->keep_cols > 0 && p->keep_cols <= p->m - 1 &&
              !one_column_tiles) ? 1 : 0;
    // per pass (TCFD_NYQ_PACK = 3: the opening pass of a call only, for A/B runs; the row pass reads either form)
    p->nyq_a = p->nyq;
    p->nyq_ca = p->nyq && p->tune.nyq_pack != 3;
    *out = p;
    return 0;
}

// ------------------------------------------------------------------ per-sample physics
// One member's linear term nu * lap - drag in the plan's real type, two rounded operations (as the tensor arithmetic that forms a
// scalar plan's table), and plan_fill's separability test on it: |l[i][j] - (lr[i] + lc[j])| <= 8 eps max|l| with
// lr[i] = l[i][0] - l[0][0], lc[j] = l[0][j] -- the pair the column kernels form for the member from lap_r / lap_c.
template <typename T>
static T member_lin(T nu, T lap, T drag) {
#pragma clang fp contract(off)
    const T prod = nu * lap;
    return prod - drag;
}
template <typename T>
static bool member_separable(const std::vector<T>& lap, int n, int m, T nu, T drag) {
    T lmax = 0;
    for (T v : lap) lmax = std::max(lmax, (T)std::fabs(member_lin(nu, v, drag)));
    const T tol = (T)8 * std::numeric_limits<T>::epsilon() * lmax;
    const T l00 = member_lin(nu, lap[0], drag);
    for (int i = 0; i < n; ++i) {
        const T lr = member_lin(nu, lap[(size_t)i * m], drag) - l00;
        for (int j = 0; j < m; ++j)
            if (std::fabs(member_lin(nu, lap[(size_t)i * m + j], drag) - (lr + member_lin(nu, lap[j], drag))) > tol) return false;
    }
    return true;
}
template <typename T>
static int ensemble_fill(tcfd_ns2d_plan* p, long count, const double* laplace, const double* nu, const double* drag,
                         const double* fscale) {
    const int n = p->n, m = p->m;
    std::vector<T> lap((size_t)n * m), lr(n), lc(m), tab(4 * (size_t)count);
    for (size_t e = 0; e < lap.size(); ++e) lap[e] = (T)laplace[e];
    for (int i = 0; i < n; ++i) lr[i] = lap[(size_t)i * m];
    for (int j = 0; j < m; ++j) lc[j] = lap[j];
    bool sep = p->sep != 0;   // the mask is separable and the tables were not forced (plan_fill)
    for (long b = 0; b < count; ++b) {
        tab[4 * b] = (T)nu[b];
        tab[4 * b + 1] = drag ? (T)drag[b] : (T)0;
        tab[4 * b + 2] = fscale ? (T)fscale[b] : (T)1;
        // derived, so that a workgroup needs no load of its own for it: the member's l[0][0], subtracted from every lin_r entry
        tab[4 * b + 3] = member_lin(tab[4 * b], lap[0], tab[4 * b + 1]);
        if (sep) sep = member_separable(lap, n, m, tab[4 * b], tab[4 * b + 1]);
    }
    int rc;
    if ((rc = upload(&p->ens, tab))) return rc;
    if ((rc = upload(&p->lap_r, lr))) return rc;
    if ((rc = upload(&p->lap_c, lc))) return rc;
    if (!sep && (rc = upload(&p->lap, lap))) return rc;
    p->ens_sep = sep ? 1 : 0;
    p->ens_count = count;
    return 0;
}

extern "C" int tcfd_ns2d_plan_set_ensemble(tcfd_ns2d_plan* p, long count, const double* laplace, const double* nu,
                                           const double* drag, const double* forcing_scale) {
    if (!p) return fail(TCFD_EINVAL, "plan_set_ensemble: null plan");
    if (count < 0) return fail(TCFD_EINVAL, "plan_set_ensemble: count %ld < 0", count);
    if (count > 0 && (!laplace || !nu)) return fail(TCFD_EINVAL, "plan_set_ensemble: laplace and nu are required when count > 0");
    if (count > 0)
        if (int rc = check_batch(p, count)) return rc;
    std::lock_guard<std::mutex> lock(p->mu);
    // a captured step holds pointers into the table: it does not outlive it
    if (GraphState* g = p->gs) {
        if (g->exec) { (void)hipGraphExecDestroy(g->exec); g->exec = nullptr; }
        if (g->graph) { (void)hipGraphDestroy(g->graph); g->graph = nullptr; }
        if (g->exec_multi) { (void)hipGraphExecDestroy(g->exec_multi); g->exec_multi = nullptr; }
        if (g->graph_multi) { (void)hipGraphDestroy(g->graph_multi); g->graph_multi = nullptr; }
        g->ens = nullptr;
    }
    // (hipFree waits for the device: no launch of an earlier call still reads the old tables)
    void** tabs[] = {&p->ens, &p->lap, &p->lap_r, &p->lap_c};
    for (void** q : tabs)
        if (*q) { (void)hipFree(*q); *q = nullptr; }
    p->ens_count = 0;
    p->ens_sep = 0;
    if (count == 0) return 0;   // a scalar plan again: the tables of plan_create
    int rc = p->dtype == TCFD_C128 ? ensemble_fill<double>(p, count, laplace, nu, drag, forcing_scale)
                                   : ensemble_fill<float>(p, count, laplace, nu, drag, forcing_scale);
    if (rc) {   // never half an ensemble
        for (void** q : tabs)
            if (*q) { (void)hipFree(*q); *q = nullptr; }
        p->ens_count = 0;
        p->ens_sep = 0;
    }
    return rc;
}

// an ensemble plan steps exactly its own members, one field each
static int check_ensemble_batch(const tcfd_ns2d_plan* p, long batch, const char* what) {
    if (p->ens_count > 0 && batch != p->ens_count)
        return fail(TCFD_EINVAL, "%s: batch %ld on a plan with per-sample parameters for %ld fields (tcfd_ns2d_plan_set_ensemble)",
                    what, batch, p->ens_count);
    return 0;
}
// the tangent-linear, adjoint and refiner kernels read ONE linear-term table
static int refuse_ensemble(const tcfd_ns2d_plan* p, const char* what) {
    if (p->ens_count > 0)
        return fail(TCFD_EINVAL, "%s: not implemented for a plan with per-sample parameters (tcfd_ns2d_plan_set_ensemble, %ld "
                    "fields): the tangent-linear, adjoint and refiner kernels read one linear-term table", what, p->ens_count);
    return 0;
}

extern "C" int tcfd_ns2d_plan_info(const tcfd_ns2d_plan* p, int* separable, int* sparse_forcing, int* keep_cols) {
    if (!p) return fail(TCFD_EINVAL, "plan_info: null plan");
    if (separable) *separable = p->sep;
    if (sparse_forcing) *sparse_forcing = p->f_sparse;
    if (keep_cols) *keep_cols = p->keep_cols;
    return 0;
}

// Fields per chunk of a batched call.  TCFD_CHUNK > 0 forces it, 0 disables chunking, -1 (default) sizes the chunk so
// that its working set -- 4 planes + advection + RK accumulator + padded state, 7 workspace fields per batch element --
// fits the 256 MB Infinity Cache (measured on MI355X, steps/s per call: 1024^2 x 64 fp64 122.7 -> 129.3 at 4 fields
// per chunk, 114.5 at 5; 512^2 x 64 fp64 408 -> 501 at 16).  Chunks are balanced.
// the seven-field working sets (4 planes + advection + RK accumulator + padded state of one field) that fit the cache
static long cache_fields(const tcfd_ns2d_plan* p) {
    const size_t per_field = 7 * (size_t)p->n * p->ldw * (p->dtype == TCFD_C128 ? 16 : 8);
    // 61/64 of the cache (244 of 256 MB, the measured optimum on MI355X: 4 fields of 1024^2 fp64 = 239 MB fit, 5 do not)
    return (long)((p->tune.cache_bytes / 64 * 61) / per_field);
}
static long chunk_fields(const tcfd_ns2d_plan* p, long batch) {
    long c = p->tune.chunk;
    if (c == 0) return batch;
    if (c < 0) {
        c = cache_fields(p);
        // fewer than 3 fields per chunk: only at 2048^2, where ONE field is a whole round of workgroups (258 column tiles) and
        // most of its working set (237 of 244 MB) still fits: 16 fields 12.8 -> 11.5 ms per step with single-field chunks; at
        // 1536^2 / 1280^2 (1 - 2 fields would fit, 194 / 162 workgroups per field) the whole batch at once is faster
        // (6.3 vs 7.9 ms, 9.3 vs 13.0 ms: tests/micro/n2048_chunk.py)
        // 4096^2: not even one field's working set fits (7 fields = 940 MB fp64 / 473 MB fp32, c = 0), so nothing of a chunk stays on
        // die whatever its size.  Four fields per chunk: measured at 4096^2 x 4 (tests/bench_ns2d_large.py, profiles/
        // ns2d_large_bench.json) the four fields in every launch step in 13.06 ms fp64 against 13.76 one field at a
        // time (a field is 4 - 8 rounds of column workgroups: longer launches amortise their tails and the launch gaps); fp32
        // shows no preference (7.91 vs 7.68 ms, the sign changing between runs).  Beyond four the scratch would grow with the
        // batch: 8 fields of the chunk, 4.3 GB fp64 at four
        if (c < 3 && p->n >= 4096) c = 4;
        else if (c < 3) return (c >= 1 && p->n >= 2048) ? 1 : batch;
        if (p->tune.round_fields > 0 && c > p->tune.round_fields) c = c / p->tune.round_fields * p->tune.round_fields;   // whole rounds
    }
    if (c >= batch) return batch;
    const long nchunks = (batch + c - 1) / c;
    return (batch + nchunks - 1) / nchunks;
}

// Scratch of the batched calls.  They run chunk by chunk through ONE chunk-sized set of 8 fields (h, adv, 4 planes,
// line-aligned state, second state), so the need does not grow with the batch beyond one chunk -- except for irfft2,
// which stages ONE field of the whole batch.  (1024^2 x 64 fp64: 0.55 GB instead of the 4.4 GB of an unchunked step.)
extern "C" size_t tcfd_ns2d_workspace_bytes(const tcfd_ns2d_plan* p, long batch) {
    if (!p || batch <= 0) return 0;
    return std::max((size_t)8 * field_bytes(p, chunk_fields(p, batch)), field_bytes(p, batch));
}

extern "C" int tcfd_ns2d_plan_chunking(const tcfd_ns2d_plan* p, long batch, long* fields_per_chunk, size_t* cache_bytes,
                                       int* cache_source) {
    if (!p || batch < 0) return fail(TCFD_EINVAL, "plan_chunking: bad argument");
    if (fields_per_chunk) *fields_per_chunk = batch > 0 ? chunk_fields(p, batch) : 0;
    if (cache_bytes) *cache_bytes = p->tune.cache_bytes;
    if (cache_source) *cache_source = p->tune.cache_source;
    return 0;
}

extern "C" int tcfd_ns2d_step_imex(const tcfd_ns2d_plan* p, const void* w_in, void* w_out, void* dwdt, long batch,
                                   int nstages, const double* fa, const double* beta, const double* gdt,
                                   const double* mu_num, const double* mu_den, const int* base0, int steps,
                                   double inv_total_dt, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w_in || !w_out || !beta || !gdt || !mu_num) return fail(TCFD_EINVAL, "step: null argument");
    if (batch <= 0 || steps <= 0 || nstages <= 0) return fail(TCFD_EINVAL, "step: batch/steps/nstages must be > 0");
    if (dwdt && w_in == w_out) return fail(TCFD_EINVAL, "step: w_out may alias w_in only when dwdt is NULL");
    if (int rce = check_ensemble_batch(p, batch, "step")) return rce;
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_workspace_bytes(p, batch));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // Batch chunking (TCFD_CHUNK = fields per chunk): the batch elements are independent, so the call may run chunk by
    // chunk -- every stage of every step of one chunk back to back, all chunks through the SAME (chunk-sized) part of
    // the workspace.  With a chunk whose working set (4 planes + adv + h + state) fits the 256 MB Infinity Cache the
    // planes written by a column pass are still on die when the row pass reads them.
    const long chunk = chunk_fields(p, batch);
    if (chunk < batch) {
        const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
        for (long b0 = 0; b0 < batch; b0 += chunk) {
            const long nb = std::min(chunk, batch - b0);
            const unsigned char* in = (const unsigned char*)w_in + b0 * esz;
            unsigned char* out = (unsigned char*)w_out + b0 * esz;
            unsigned char* dw = dwdt ? (unsigned char*)dwdt + b0 * esz : nullptr;
            rc = NS2D_SIZED(p, step, p, in, out, dw, nb, nstages, beta, gdt, mu_num, fa, mu_den, base0, steps, inv_total_dt, ws, st, b0);
            if (rc) return rc;
        }
        return 0;
    }
    return NS2D_SIZED(p, step, p, w_in, w_out, dwdt, batch, nstages, beta, gdt, mu_num, fa, mu_den, base0, steps, inv_total_dt, ws,
                      st, 0L);
}

extern "C" int tcfd_ns2d_step(const tcfd_ns2d_plan* p, const void* w_in, void* w_out, void* dwdt, long batch,
                              int nstages, const double* beta, const double* gdt, const double* mu, int steps,
                              double inv_total_dt, void* ws, size_t ws_bytes, void* stream) {
    return tcfd_ns2d_step_imex(p, w_in, w_out, dwdt, batch, nstages, nullptr, beta, gdt, mu, nullptr, nullptr, steps,
                               inv_total_dt, ws, ws_bytes, stream);
}

// F(w) / residual sweeps chunk by chunk like the steps (the planes of a chunk stay on die between the two passes)
int ns2d::explicit_chunked(const tcfd_ns2d_plan* p, const void* w, void* out, const void* wt, void* psi, bool residual,
                           long batch, void* ws, hipStream_t st) {
    const long chunk = chunk_fields(p, batch);
    if (chunk >= batch) return NS2D_SIZED(p, explicit_terms, p, w, out, wt, psi, residual, batch, ws, st, 0L);
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    auto at = [&](const void* base, long b0) -> unsigned char* {
        return base ? (unsigned char*)base + (size_t)b0 * esz : nullptr;
    };
    for (long b0 = 0; b0 < batch; b0 += chunk) {
        const long nb = std::min(chunk, batch - b0);
        int rc = NS2D_SIZED(p, explicit_terms, p, at(w, b0), at(out, b0), at(wt, b0), at(psi, b0), residual, nb, ws, st, b0);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int tcfd_ns2d_explicit_terms(const tcfd_ns2d_plan* p, const void* w, void* out, long batch, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (!p || !w || !out || batch <= 0) return fail(TCFD_EINVAL, "explicit_terms: bad argument");
    if (int rce = check_ensemble_batch(p, batch, "explicit_terms")) return rce;
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_workspace_bytes(p, batch));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ns2d::explicit_chunked(p, w, out, nullptr, nullptr, false, batch, ws, st);
}

extern "C" int tcfd_ns2d_explicit_terms_vjp(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, long batch,
                                            void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || !gm || !xout || batch <= 0) return fail(TCFD_EINVAL, "explicit_terms_vjp: bad argument");
    if (int rce = refuse_ensemble(p, "explicit_terms_vjp")) return rce;
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_workspace_bytes(p, batch));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    const size_t xs = (size_t)batch * p->n * p->m;            // elements between the four outputs
    const long chunk = chunk_fields(p, batch);
    for (long b0 = 0; b0 < batch; b0 += chunk) {
        const long nb = std::min(chunk, batch - b0);
        rc = NS2D_SIZED(p, explicit_vjp, p, (const unsigned char*)w + (size_t)b0 * esz, (const unsigned char*)gm + (size_t)b0 * esz,
                        (unsigned char*)xout + (size_t)b0 * esz, xs, nb, ws, st);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ tangent-linear model (forward-mode JVP)
// a chunk of the tangent calls holds twice the fields of a chunk of the plain step
static long jvp_chunk_fields(const tcfd_ns2d_plan* p, long batch) {
    const long c2 = chunk_fields(p, 2 * batch);
    if (c2 >= 2 * batch) return batch;
    const long c = std::max<long>(1, c2 / 2);
    if (c >= batch) return batch;
    const long nchunks = (batch + c - 1) / c;
    return (batch + nchunks - 1) / nchunks;
}
extern "C" size_t tcfd_ns2d_jvp_workspace_bytes(const tcfd_ns2d_plan* p, long batch) {
    if (!p || batch <= 0) return 0;
    return (size_t)16 * field_bytes(p, jvp_chunk_fields(p, batch));
}

extern "C" int tcfd_ns2d_explicit_terms_jvp(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f, void* out_df,
                                            long batch, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || !dw || !out_df || batch <= 0) return fail(TCFD_EINVAL, "explicit_terms_jvp: bad argument");
    if (int rce = refuse_ensemble(p, "explicit_terms_jvp")) return rce;
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_jvp_workspace_bytes(p, batch));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    const long chunk = jvp_chunk_fields(p, batch);
    for (long b0 = 0; b0 < batch; b0 += chunk) {
        const long nb = std::min(chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        rc = NS2D_SIZED(p, explicit_jvp, p, (const unsigned char*)w + o, (const unsigned char*)dw + o,
                        out_f ? (unsigned char*)out_f + o : nullptr, (unsigned char*)out_df + o, nb, ws, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int tcfd_ns2d_step_jvp(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out,
                                  long batch, int nstages, const double* fa, const double* beta, const double* gdt,
                                  const double* mu_num, const double* mu_den, const int* base0, int steps, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (!p || !w_in || !dw_in || !w_out || !dw_out || !beta || !gdt || !mu_num) return fail(TCFD_EINVAL, "step_jvp: null argument");
    if (batch <= 0 || steps <= 0 || nstages <= 0) return fail(TCFD_EINVAL, "step_jvp: batch/steps/nstages must be > 0");
    if (int rce = refuse_ensemble(p, "step_jvp")) return rce;
    if (w_out == dw_out || w_out == dw_in || dw_out == w_in)
        return fail(TCFD_EINVAL, "step_jvp: the state and the tangent arrays must not overlap");
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_jvp_workspace_bytes(p, batch));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    const long chunk = jvp_chunk_fields(p, batch);
    for (long b0 = 0; b0 < batch; b0 += chunk) {
        const long nb = std::min(chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        rc = NS2D_SIZED(p, step_jvp, p, (const unsigned char*)w_in + o, (const unsigned char*)dw_in + o, (unsigned char*)w_out + o,
                        (unsigned char*)dw_out + o, nb, nstages, fa, beta, gdt, mu_num, mu_den, base0, steps, ws, st);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ tangent bundle: one state, K tangents per call
// Fields per chunk and tangents per group.  A chunk of c states is in flight with its own plane set and those of kg tangents:
// (1 + kg) c of the 7-field working sets chunk_fields sizes the cache for (`cap` of them fit; TCFD_CHUNK > 0 sets cap, 0 turns
// chunking off).
//   cap >= K + 1 : every tangent in one group, c = cap / (K + 1) states per chunk (balanced) -- K = 1 is jvp_chunk_fields' rule
//   2 <= cap < K + 1 : one state per chunk, kg = cap - 1 tangents per group (balanced): the state's planes stay on die while the
//                  groups pass, its column pass runs once per stage and its row transforms once per group
//   cap < 2      : nothing stays on die whatever the grouping (n >= 1280 in fp64, n >= 2048 in fp32): one state, one group
// The scratch is bundle_fields(K, kg) chunk-sized fields.
struct BundleShape { long chunk; int kg; };
constexpr int BUNDLE_MAX_TANGENTS = 65535;
// the largest chunk and group the rule allows (a call balances both below these)
static BundleShape bundle_limits(const tcfd_ns2d_plan* p, long batch, int ntan) {
    long cap = p->tune.chunk;
    if (cap == 0) return {batch, ntan};
    if (cap < 0) cap = cache_fields(p);      // chunk_fields' budget
    if (cap >= (long)ntan + 1) return {std::min(batch, cap / (ntan + 1)), ntan};
    if (cap >= 2) return {1, (int)(cap - 1)};
    return {1, ntan};
}
static BundleShape bundle_shape(const tcfd_ns2d_plan* p, long batch, int ntan) {
    const BundleShape lim = bundle_limits(p, batch, ntan);
    auto balanced = [](long total, long per) {
        const long parts = (total + per - 1) / per;
        return (total + parts - 1) / parts;
    };
    return {balanced(batch, lim.chunk), (int)balanced(ntan, lim.kg)};
}

// What the rule's limits need, and never less than a call with fewer tangents needs: the chunk shrinks as K grows, so the product
// fields x chunk is not monotone by itself -- a caller who sizes one buffer for its largest bundle can rely on it for every smaller one.
extern "C" size_t tcfd_ns2d_bundle_workspace_bytes(const tcfd_ns2d_plan* p, long batch, int ntangents) {
    if (!p || batch <= 0 || ntangents < 1 || ntangents > BUNDLE_MAX_TANGENTS) return 0;
    size_t need = 0;
    for (int k = 1; k <= ntangents; ++k) {
        const BundleShape lim = bundle_limits(p, batch, k);
        need = std::max(need, (size_t)bundle_fields(k, lim.kg) * field_bytes(p, lim.chunk));
    }
    return need;
}

static bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const unsigned char *a0 = (const unsigned char*)a, *b0 = (const unsigned char*)b;
    return a0 < b0 + bn && b0 < a0 + an;
}
// the checks the two bundle calls share after their null / count checks; the launches of one chunk hold (kg + 1) * chunk fields at most
static int check_bundle(const tcfd_ns2d_plan* p, const char* what, long batch, int ntangents, void* ws, size_t ws_bytes) {
    if (ntangents < 1 || ntangents > BUNDLE_MAX_TANGENTS)
        return fail(TCFD_EINVAL, "%s: ntangents must be in [1, %d] (got %d)", what, BUNDLE_MAX_TANGENTS, ntangents);
    if (int rce = refuse_ensemble(p, what)) return rce;
    if (batch > max_batch(p) / ntangents)
        return fail(TCFD_EINVAL, "%s: batch %ld x %d tangents exceeds the largest batch of one call at n = %d (%ld fields)", what,
                    batch, ntangents, p->n, max_batch(p));
    return check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_bundle_workspace_bytes(p, batch, ntangents));
}

extern "C" int tcfd_ns2d_explicit_terms_jvp_bundle(const tcfd_ns2d_plan* p, const void* w, const void* dw, void* out_f,
                                                   void* out_df, long batch, int ntangents, void* ws, size_t ws_bytes,
                                                   void* stream) {
    if (!p || !w || !dw || !out_df || batch <= 0) return fail(TCFD_EINVAL, "explicit_terms_jvp_bundle: bad argument");
    if (int rc = check_bundle(p, "explicit_terms_jvp_bundle", batch, ntangents, ws, ws_bytes)) return rc;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    const size_t sb = (size_t)batch * esz, tb = (size_t)ntangents * sb;
    // the groups of a chunk and the chunks of a call run one after the other: an output that overlapped an input would be read back
    if (ranges_overlap(out_df, tb, w, sb) || ranges_overlap(out_df, tb, dw, tb) ||
        (out_f && (ranges_overlap(out_f, sb, w, sb) || ranges_overlap(out_f, sb, dw, tb) || ranges_overlap(out_f, sb, out_df, tb))))
        return fail(TCFD_EINVAL, "explicit_terms_jvp_bundle: the outputs must not overlap the inputs or each other");
    hipStream_t st = (hipStream_t)stream;
    const BundleShape sh = bundle_shape(p, batch, ntangents);
    const size_t ts = (size_t)batch * p->n * p->m;      // elements between two tangents
    for (long b0 = 0; b0 < batch; b0 += sh.chunk) {
        const long nb = std::min(sh.chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        int rc = NS2D_SIZED(p, explicit_jvp_bundle, p, (const unsigned char*)w + o, (const unsigned char*)dw + o,
                            out_f ? (unsigned char*)out_f + o : nullptr, (unsigned char*)out_df + o, ts, nb, ntangents, sh.kg, ws, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int tcfd_ns2d_step_jvp_bundle(const tcfd_ns2d_plan* p, const void* w_in, const void* dw_in, void* w_out, void* dw_out,
                                         long batch, int ntangents, int nstages, const double* fa, const double* beta,
                                         const double* gdt, const double* mu_num, const double* mu_den, const int* base0,
                                         int steps, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w_in || !dw_in || !w_out || !dw_out || !beta || !gdt || !mu_num)
        return fail(TCFD_EINVAL, "step_jvp_bundle: null argument");
    if (batch <= 0 || steps <= 0 || nstages <= 0) return fail(TCFD_EINVAL, "step_jvp_bundle: batch/steps/nstages must be > 0");
    if (int rc = check_bundle(p, "step_jvp_bundle", batch, ntangents, ws, ws_bytes)) return rc;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    const size_t sb = (size_t)batch * esz, tb = (size_t)ntangents * sb;
    // a state array and a tangent array never share memory; an output may BE its input (in place: every element is read before it
    // is written, by the same thread), but not overlap it shifted -- a later chunk would read what an earlier one wrote
    if (ranges_overlap(w_out, sb, dw_out, tb) || ranges_overlap(w_out, sb, dw_in, tb) || ranges_overlap(dw_out, tb, w_in, sb) ||
        ranges_overlap(w_in, sb, dw_in, tb))
        return fail(TCFD_EINVAL, "step_jvp_bundle: the state and the tangent arrays must not overlap");
    if ((w_out != w_in && ranges_overlap(w_out, sb, w_in, sb)) || (dw_out != dw_in && ranges_overlap(dw_out, tb, dw_in, tb)))
        return fail(TCFD_EINVAL, "step_jvp_bundle: an output overlaps its input without being it (identical or disjoint)");
    hipStream_t st = (hipStream_t)stream;
    const BundleShape sh = bundle_shape(p, batch, ntangents);
    const size_t ts = (size_t)batch * p->n * p->m;
    for (long b0 = 0; b0 < batch; b0 += sh.chunk) {
        const long nb = std::min(sh.chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        int rc = NS2D_SIZED(p, step_jvp_bundle, p, (const unsigned char*)w_in + o, (const unsigned char*)dw_in + o,
                            (unsigned char*)w_out + o, (unsigned char*)dw_out + o, ts, nb, ntangents, sh.kg, nstages, fa, beta, gdt,
                            mu_num, mu_den, base0, steps, ws, st);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ adjoint model (reverse of the fused step)
// Chunks as the plain step's (the sweeps of a reversed stage are the forward sweep and the explicit terms' VJP, whose working
// sets are the step's); 12 + nstages chunk-sized fields (VjpWs).
extern "C" size_t tcfd_ns2d_step_vjp_workspace_bytes(const tcfd_ns2d_plan* p, long batch, int nstages) {
    if (!p || batch <= 0 || nstages <= 0 || nstages > VJP_MAX_STAGES) return 0;
    return (size_t)vjp_fields(nstages) * field_bytes(p, chunk_fields(p, batch));
}

extern "C" int tcfd_ns2d_step_vjp(const tcfd_ns2d_plan* p, const void* saved, const void* g_out, const void* pre, const void* post,
                                  void* g_in, long batch, int nstages, const double* fa, const double* beta, const double* gdt,
                                  const double* mu_num, const double* mu_den, const int* base0, int steps, void* ws,
                                  size_t ws_bytes, void* stream) {
    if (!p || !saved || !g_out || !pre || !post || !g_in || !beta || !gdt || !mu_num)
        return fail(TCFD_EINVAL, "step_vjp: null argument");
    if (batch <= 0) return fail(TCFD_EINVAL, "step_vjp: batch must be > 0");
    if (int rce = refuse_ensemble(p, "step_vjp")) return rce;
    if (steps <= 0) return fail(TCFD_EINVAL, "step_vjp: steps must be > 0 (got %d)", steps);
    if (nstages <= 0 || nstages > VJP_MAX_STAGES)
        return fail(TCFD_EINVAL, "step_vjp: nstages %d out of range [1, %d]", nstages, VJP_MAX_STAGES);
    // (a short workspace is TCFD_EWORKSPACE, as for every call that takes one: include/tcfd.h, Conventions)
    if (int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_step_vjp_workspace_bytes(p, batch, nstages))) return rc;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;      // bytes of one field, caller layout
    {
        const unsigned char *s0 = (const unsigned char*)saved, *s1 = s0 + (size_t)steps * batch * esz;
        const unsigned char *g0 = (const unsigned char*)g_in, *g1 = g0 + (size_t)batch * esz;
        if (g0 < s1 && s0 < g1) return fail(TCFD_EINVAL, "step_vjp: g_in overlaps saved (the saved states are read to the end)");
        // g_in == g_out is in place (every chunk reads its own part of g_out first); a shifted overlap would let a later chunk read
        // what an earlier one wrote
        const unsigned char* o0 = (const unsigned char*)g_out;
        if (g0 != o0 && g0 < o0 + (size_t)batch * esz && o0 < g1)
            return fail(TCFD_EINVAL, "step_vjp: g_in overlaps g_out without being g_out (identical or disjoint)");
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t step_stride = (size_t)batch * p->n * p->m;      // elements between saved[s] and saved[s + 1]
    const long chunk = chunk_fields(p, batch);
    for (long b0 = 0; b0 < batch; b0 += chunk) {
        const long nb = std::min(chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        int rc = NS2D_SIZED(p, step_vjp, p, (const unsigned char*)saved + o, step_stride, (const unsigned char*)g_out + o, pre, post,
                            (unsigned char*)g_in + o, nb, nstages, fa, beta, gdt, mu_num, mu_den, base0, steps, ws, st);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------ adjoint model for a bundle of K cotangents per trajectory
// Chunks and cotangent groups as the tangent bundle's (bundle_shape: the state's plane set and kg cotangent sets in flight are the
// same cache budget); cobundle_fields chunk-sized fields, and never less than a call with fewer cotangents needs.
extern "C" size_t tcfd_ns2d_step_vjp_bundle_workspace_bytes(const tcfd_ns2d_plan* p, long batch, int ncotangents, int nstages) {
    if (!p || batch <= 0 || ncotangents < 1 || ncotangents > BUNDLE_MAX_TANGENTS || nstages <= 0 || nstages > VJP_MAX_STAGES) return 0;
    size_t need = 0;
    for (int k = 1; k <= ncotangents; ++k) {
        const BundleShape lim = bundle_limits(p, batch, k);
        need = std::max(need, (size_t)cobundle_fields(k, lim.kg, nstages) * field_bytes(p, lim.chunk));
    }
    return need;
}

// the checks the two cotangent-bundle calls share after their null checks
static int check_cobundle(const tcfd_ns2d_plan* p, const char* what, long batch, int ncot, int nstages, void* ws, size_t ws_bytes) {
    if (batch <= 0) return fail(TCFD_EINVAL, "%s: batch must be > 0", what);
    if (ncot < 1 || ncot > BUNDLE_MAX_TANGENTS)
        return fail(TCFD_EINVAL, "%s: ncotangents must be in [1, %d] (got %d)", what, BUNDLE_MAX_TANGENTS, ncot);
    if (int rce = refuse_ensemble(p, what)) return rce;
    if (nstages <= 0 || nstages > VJP_MAX_STAGES)
        return fail(TCFD_EINVAL, "%s: nstages %d out of range [1, %d]", what, nstages, VJP_MAX_STAGES);
    if (batch > max_batch(p) / ncot)
        return fail(TCFD_EINVAL, "%s: batch %ld x %d cotangents exceeds the largest batch of one call at n = %d (%ld fields)", what,
                    batch, ncot, p->n, max_batch(p));
    return check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_step_vjp_bundle_workspace_bytes(p, batch, ncot, nstages));
}

extern "C" int tcfd_ns2d_explicit_terms_vjp_bundle(const tcfd_ns2d_plan* p, const void* w, const void* gm, void* xout, long batch,
                                                   int ncotangents, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || !gm || !xout) return fail(TCFD_EINVAL, "explicit_terms_vjp_bundle: null argument");
    if (int rc = check_cobundle(p, "explicit_terms_vjp_bundle", batch, ncotangents, 1, ws, ws_bytes)) return rc;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;
    const size_t sb = (size_t)batch * esz, cb = (size_t)ncotangents * sb;
    // the groups of a chunk and the chunks of a call run one after the other: an output that overlapped an input would be read back
    if (ranges_overlap(xout, 4 * cb, w, sb) || ranges_overlap(xout, 4 * cb, gm, cb))
        return fail(TCFD_EINVAL, "explicit_terms_vjp_bundle: xout must not overlap w or gm");
    hipStream_t st = (hipStream_t)stream;
    const BundleShape sh = bundle_shape(p, batch, ncotangents);
    const size_t cs = (size_t)batch * p->n * p->m;      // elements between two cotangents
    for (long b0 = 0; b0 < batch; b0 += sh.chunk) {
        const long nb = std::min(sh.chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        int rc = NS2D_SIZED(p, explicit_vjp_bundle, p, (const unsigned char*)w + o, (const unsigned char*)gm + o,
                            (unsigned char*)xout + o, cs, nb, ncotangents, sh.kg, ws, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int tcfd_ns2d_step_vjp_bundle(const tcfd_ns2d_plan* p, const void* saved, const void* g_out, const void* pre,
                                         const void* post, void* g_in, long batch, int ncotangents, int nstages, const double* fa,
                                         const double* beta, const double* gdt, const double* mu_num, const double* mu_den,
                                         const int* base0, int steps, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !saved || !g_out || !pre || !post || !g_in || !beta || !gdt || !mu_num)
        return fail(TCFD_EINVAL, "step_vjp_bundle: null argument");
    if (steps <= 0) return fail(TCFD_EINVAL, "step_vjp_bundle: steps must be > 0 (got %d)", steps);
    if (int rc = check_cobundle(p, "step_vjp_bundle", batch, ncotangents, nstages, ws, ws_bytes)) return rc;
    const size_t esz = (p->dtype == TCFD_C128 ? 16 : 8) * (size_t)p->n * p->m;      // bytes of one field, caller layout
    const size_t sb = (size_t)batch * esz, cb = (size_t)ncotangents * sb;
    if (ranges_overlap(g_in, cb, saved, (size_t)steps * sb))
        return fail(TCFD_EINVAL, "step_vjp_bundle: g_in overlaps saved (the saved states are read to the end)");
    // g_in == g_out is in place (every chunk reads its own part of g_out first); a shifted overlap would let a later chunk read
    // what an earlier one wrote
    if (g_in != g_out && ranges_overlap(g_in, cb, g_out, cb))
        return fail(TCFD_EINVAL, "step_vjp_bundle: g_in overlaps g_out without being g_out (identical or disjoint)");
    hipStream_t st = (hipStream_t)stream;
    const BundleShape sh = bundle_shape(p, batch, ncotangents);
    const size_t cs = (size_t)batch * p->n * p->m;      // elements between saved[s] and saved[s + 1], and between two cotangents
    for (long b0 = 0; b0 < batch; b0 += sh.chunk) {
        const long nb = std::min(sh.chunk, batch - b0);
        const size_t o = (size_t)b0 * esz;
        int rc = NS2D_SIZED(p, step_vjp_bundle, p, (const unsigned char*)saved + o, cs, (const unsigned char*)g_out + o, pre, post,
                            (unsigned char*)g_in + o, cs, nb, ncotangents, sh.kg, nstages, fa, beta, gdt, mu_num, mu_den, base0, steps,
                            ws, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int tcfd_ns2d_stream_residual(const tcfd_ns2d_plan* p, const void* w, const void* wt, void* psi,
                                         void* residual, long batch, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !w || batch <= 0 || (residual && !wt)) return fail(TCFD_EINVAL, "stream_residual: bad argument");
    if (int rce = check_ensemble_batch(p, batch, "stream_residual")) return rce;
    int rc = check_ws(p, batch, ws, ws_bytes, tcfd_ns2d_workspace_bytes(p, batch));
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ns2d::explicit_chunked(p, w, residual, wt, psi, true, batch, ws, st);
}

// ------------------------------------------------------------------ small elementwise kernels
template <typename T>
__global__ void k_velocity(const cx<T>* __restrict__ w, cx<T>* __restrict__ uh, cx<T>* __restrict__ vh,
                           cx<T>* __restrict__ psi, const T* __restrict__ kxs, const T* __restrict__ kys, int n,
                           int m, size_t count) {
    constexpr T TWO_PI = (T)6.283185307179586476925286766559;
    constexpr T M4PI2 = (T)(-39.478417604357434475337963999505);
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < count;
         idx += (size_t)gridDim.x * blockDim.x) {
        const int jc = (int)(idx % m);
        const int i = (int)((idx / m) % n);
        const T kx = kxs[i], ky = kys[jc];
        T lap = M4PI2 * (kx * kx + ky * ky);
        if (i == 0 && jc == 0) lap = (T)1;
        const cx<T> p = cscale(w[idx], (T)-1 / lap);
        if (psi) psi[idx] = p;
        if (uh) uh[idx] = mul_i(cscale(p, TWO_PI * ky));
        if (vh) vh[idx] = mul_mi(cscale(p, TWO_PI * kx));
    }
}

template <typename T>
static int velocity_impl(const tcfd_ns2d_plan* p, const void* w, void* uh, void* vh, void* psi, long batch,
                         hipStream_t st) {
    const size_t count = (size_t)batch * p->n * p->m;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 4096);
    hipLaunchKernelGGL(k_velocity<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)w, (cx<T>*)uh, (cx<T>*)vh,
                       (cx<T>*)psi, (const T*)p->kx, (const T*)p->ky, p->n, p->m, count);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int tcfd_ns2d_velocity(const tcfd_ns2d_plan* p, const void* w, void* uh, void* vh, void* psi, long batch,
                                  void* stream) {
    if (!p || !w || batch <= 0) return fail(TCFD_EINVAL, "velocity: bad argument");
    if (int rc = check_batch(p, batch)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return p->dtype == TCFD_C128 ? velocity_impl<double>(p, w, uh, vh, psi, batch, st)
                                 : velocity_impl<float>(p, w, uh, vh, psi, batch, st);
}

// ------------------------------------------------------------------ weighted squared norm of half spectra
// partial[b][blk] = sum over the block's share of field b of  |z[b][e]|^2 * w2[e]   (double accumulation): the
// Fourier-domain norm of SobolevLoss (fno/losses.py:263-315) in ONE pass over the spectrum instead of five
// element-wise / reduction launches.
template <typename T>
__global__ __launch_bounds__(256) void k_weighted_sqnorm(const cx<T>* __restrict__ z, const T* __restrict__ w2,
                                                         double* __restrict__ partial, long elems, int blocks) {
    __shared__ double sh[4];
    // one-dimensional grid of batch * blocks workgroups (grid.y stops at 65535 fields; b * T of a loss has no such bound)
    const long b = blockIdx.x / blocks;
    const int blk = blockIdx.x - (unsigned)(b * blocks);
    const cx<T>* zb = z + (size_t)b * elems;
    double acc = 0.0;
    for (long e = (long)blk * 256 + threadIdx.x; e < elems; e += (long)blocks * 256) {
        const cx<T> v = zb[e];
        acc += (double)((v.x * v.x + v.y * v.y) * w2[e]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

extern "C" int tcfd_weighted_sqnorm(const void* z, const void* w2, void* partial, long batch, long elems, int blocks,
                                    int dtype, void* stream) {
    if (!z || !w2 || !partial || batch <= 0 || elems <= 0 || blocks <= 0)
        return fail(TCFD_EINVAL, "weighted_sqnorm: bad argument");
    if (dtype != TCFD_C64 && dtype != TCFD_C128) return fail(TCFD_EINVAL, "weighted_sqnorm: bad dtype %d", dtype);
    if ((double)batch * blocks >= 2147483647.0) return fail(TCFD_EINVAL, "weighted_sqnorm: batch * blocks exceeds the grid limit");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(batch * blocks));
    if (dtype == TCFD_C128)
        hipLaunchKernelGGL(k_weighted_sqnorm<double>, grid, dim3(256), 0, st, (const cx<double>*)z, (const double*)w2,
                           (double*)partial, elems, blocks);
    else
        hipLaunchKernelGGL(k_weighted_sqnorm<float>, grid, dim3(256), 0, st, (const cx<float>*)z, (const float*)w2,
                           (double*)partial, elems, blocks);
    HIP_TRY(hipGetLastError());
    return 0;
}

// largest factor tcfd_irfft2_subsample accepts for this plan (the lanes of one row transform, 64 at most); < 0: bad plan
extern "C" int tcfd_irfft2_subsample_max_factor(const tcfd_ns2d_plan* p) {
    if (!p) return fail(TCFD_EINVAL, "irfft2_subsample_max_factor: null plan");
    return NS2D_SIZED(p, irfft2_sub_max, p);
}
extern "C" int tcfd_irfft2_subsample(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, int factor, void* ws,
                                   size_t ws_bytes, void* stream) {
    if (!p || !xh || !out || batch <= 0) return fail(TCFD_EINVAL, "irfft2_subsample: bad argument");
    if (factor < 2 || p->n % factor) return fail(TCFD_EINVAL, "irfft2_subsample: factor %d does not divide n = %d", factor, p->n);
    int rc = check_ws(p, batch, ws, ws_bytes, field_bytes(p, batch));
    if (rc) return rc;
    return NS2D_SIZED(p, irfft2_sub, p, xh, out, batch, factor, ws, (hipStream_t)stream);
}

extern "C" int tcfd_rfft2(const tcfd_ns2d_plan* p, const void* x, void* out, long batch, void* stream) {
    if (!p || !x || !out || batch <= 0) return fail(TCFD_EINVAL, "rfft2: bad argument");
    if (int rc = check_batch(p, batch)) return rc;
    return NS2D_SIZED(p, rfft2, p, x, out, batch, (hipStream_t)stream);
}

extern "C" int tcfd_irfft2(const tcfd_ns2d_plan* p, const void* xh, void* out, long batch, void* ws, size_t ws_bytes,
                           void* stream) {
    if (!p || !xh || !out || batch <= 0) return fail(TCFD_EINVAL, "irfft2: bad argument");
    int rc = check_ws(p, batch, ws, ws_bytes, field_bytes(p, batch));
    if (rc) return rc;
    return NS2D_SIZED(p, irfft2, p, xh, out, batch, ws, (hipStream_t)stream);
}

extern "C" int tcfd_ns2d_plan_variant(const tcfd_ns2d_plan* p, int* split, int* rows_kernel) {
    if (!p) return fail(TCFD_EINVAL, "plan_variant: null plan");
    return NS2D_SIZED(p, variant, p, split, rows_kernel);
}

// ------------------------------------------------------------------ test hook: the cross-lane transform alone
// One 128-lane group transforms `count` independent 1024-point sequences (complex128).  dir = +1: natural-order
// input, output in the permutation pi of xl_fft1024 (element t of lane j at out[seq][128 t + j]); dir = -1: input in
// that layout, natural-order output.  tests/test_ns2d_gpu.py checks both against numpy through the map of pi.
template <int DIR>
__global__ __launch_bounds__(128) void k_debug_xl(const cx<double>* __restrict__ in, cx<double>* __restrict__ out,
                                                  const cx<double>* __restrict__ tw) {
    __shared__ __attribute__((aligned(16))) cx<double> lds[1024];
    const int j = threadIdx.x;
    const XlTw<double> xtw = xl_load_tw<double>(tw, j);
    cx<double> x[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) x[t] = in[(size_t)blockIdx.x * 1024 + 128 * t + j];
    NoHook nohook;
    xl_fft1024<double, DIR, 1>(x, lds, xtw, j, nohook);
#pragma unroll
    for (int t = 0; t < 8; ++t) out[(size_t)blockIdx.x * 1024 + 128 * t + j] = x[t];
}

extern "C" int tcfd_debug_xl_fft1024(const tcfd_ns2d_plan* p, const void* in, void* out, int count, int dir, void* stream) {
    if (!p || !in || !out || count <= 0 || (dir != 1 && dir != -1)) return fail(TCFD_EINVAL, "debug_xl_fft1024: bad argument");
    if (p->n != 1024 || p->dtype != TCFD_C128) return fail(TCFD_EINVAL, "debug_xl_fft1024: needs a 1024^2 complex128 plan");
    hipStream_t st = (hipStream_t)stream;
    if (dir > 0)
        hipLaunchKernelGGL(k_debug_xl<+1>, dim3(count), dim3(128), 0, st, (const cx<double>*)in, (cx<double>*)out,
                           (const cx<double>*)p->tw);
    else
        hipLaunchKernelGGL(k_debug_xl<-1>, dim3(count), dim3(128), 0, st, (const cx<double>*)in, (cx<double>*)out,
                           (const cx<double>*)p->tw);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ profiling side-car
extern "C" int tcfd_ns2d_profile_begin(tcfd_ns2d_plan* p, int max_records) {
    if (!p || max_records <= 0) return fail(TCFD_EINVAL, "profile_begin: bad argument");
    if (!p->prof) p->prof = new ProfState();
    for (auto& r : p->prof->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    p->prof->recs.clear();
    p->prof->recs.reserve(max_records);
    p->prof->max_records = max_records;
    p->prof->on = true;
    return 0;
}

extern "C" int tcfd_ns2d_profile_end(tcfd_ns2d_plan* p, int capacity, int* count, int* kinds, float* ms) {
    if (!p || !p->prof || !count) return fail(TCFD_EINVAL, "profile_end: profiling was not started");
    ProfState* ps = p->prof;
    ps->on = false;
    int n = 0;
    for (auto& r : ps->recs) {
        HIP_TRY(hipEventSynchronize(r.e1));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, r.e0, r.e1));
        if (n < capacity && kinds && ms) { kinds[n] = r.kind; ms[n] = t; }
        ++n;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    ps->recs.clear();
    *count = n;
    return 0;
}

// ---------------------------------------------------------------- HBM probe (bench.py reports it beside the 8 TB/s spec)
__global__ __launch_bounds__(256) void k_probe(const double2* __restrict__ src, double2* __restrict__ dst, size_t n16,
                                               int mode) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (mode == 0) {
        for (; i < n16; i += stride) dst[i] = src[i];
    } else if (mode == 1) {
        double acc = 0.0;
        for (; i < n16; i += stride) { const double2 v = src[i]; acc += v.x + v.y; }
        if (acc == 1.2345e300) reinterpret_cast<double*>(dst)[0] = acc;   // keeps the loads alive, never true
    } else {
        const double2 z = make_double2(0.0, 0.0);
        for (; i < n16; i += stride) dst[i] = z;
    }
}

extern "C" int tcfd_hbm_probe(const void* src, void* dst, size_t bytes, int mode, int iters, float* ms, void* stream) {
    if (!dst || (mode != 2 && !src) || !ms || bytes < 16 || bytes % 16 || iters < 1 || mode < 0 || mode > 2)
        return fail(TCFD_EINVAL, "hbm_probe: bad argument");
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    const size_t n16 = bytes / 16;
    const unsigned blocks = 256 * 16;  // 16 workgroups per CU, grid-stride
    hipLaunchKernelGGL(k_probe, dim3(blocks), dim3(256), 0, st, (const double2*)src, (double2*)dst, n16, mode);  // warm-up
    HIP_TRY(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(k_probe, dim3(blocks), dim3(256), 0, st, (const double2*)src, (double2*)dst, n16, mode);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIP_TRY(hipGetLastError());
    *ms = t / iters;
    return 0;
}

// ---------------------------------------------------------------- strided device -> host copy of record slabs
// One record of `rows` samples lands in a host array whose sample pitch is a whole trajectory: a pitched copy on the caller's
// stream (asynchronous when the host side is page-locked), so the hand-over of a record overlaps the steps that follow it.
extern "C" int tcfd_copy_rows_to_host(void* dst_host, size_t dst_pitch, const void* src_dev, size_t src_pitch,
                                      size_t row_bytes, size_t rows, void* stream) {
    if (!dst_host || !src_dev || row_bytes == 0 || dst_pitch < row_bytes || src_pitch < row_bytes)
        return fail(TCFD_EINVAL, "copy_rows_to_host: bad argument");
    if (rows == 0) return 0;
    HIP_TRY(hipMemcpy2DAsync(dst_host, dst_pitch, src_dev, src_pitch, row_bytes, rows, hipMemcpyDeviceToHost,
                             (hipStream_t)stream));
    return 0;
}

// Page-lock / release a range of ordinary host memory (hipHostRegister): the record hand-over locks the result of an
// ensemble job region by region on a helper thread -- ONE page-locked allocation of the whole result holds the runtime's
// memory lock for its full duration (0.36 s at 5.4 GB) and stalls every hipMalloc of the stepping thread behind it.
extern "C" int tcfd_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return fail(TCFD_EINVAL, "host_register: bad argument");
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return 0;
}
extern "C" int tcfd_host_unregister(void* ptr) {
    if (!ptr) return fail(TCFD_EINVAL, "host_unregister: null pointer");
    HIP_TRY(hipHostUnregister(ptr));
    return 0;
}

// ---------------------------------------------------------------- stage bookkeeping of the DIFFERENTIABLE step
// With constant coefficients a stage of the low-storage RK / Crank-Nicolson schedule is linear in (f, h_prev, b):
//     h = fa f + beta h_prev ,    u = (b + gdt h + mu L b) / (1 - mud L)            (L: the real (n, m) linear term)
// -- written exactly as the fused forward kernels write it (k_cols, MODE_C), so a differentiable trajectory reproduces the
// plain one to round-off.  autograd.py ran this as ~10 element-wise tensor launches forward and ~20 backward per stage; these
// two kernels are the stage and its vector-Jacobian product in one launch each:
//     G = g_h + gdt r (.) g_u ,   g_f = fa G ,   g_hprev = beta G ,   g_b = (1 + mu L) r (.) g_u ,      r = 1 / (1 - mud L).
// (k_stage_update: tcfd_ns2d_plan.hpp -- the recomputation of tcfd_ns2d_step_vjp in the sized units launches it too.)
template <typename T>
__global__ __launch_bounds__(256) void k_stage_update_vjp(const cx<T>* __restrict__ gu, const cx<T>* __restrict__ gh,
                                                          const T* __restrict__ Lt, T fa, T beta, T gdt, T mu, T mud,
                                                          cx<T>* __restrict__ gf, cx<T>* __restrict__ ghp,
                                                          cx<T>* __restrict__ gb, long total, long plane) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const T L = Lt[e % plane];
        const cx<T> g = cscale(gu[e], fast_rcp((T)1 - mud * L));     // r (.) g_u
        cx<T> G = cscale(g, gdt);
        if (gh) G = G + gh[e];
        gf[e] = cscale(G, fa);
        if (ghp) ghp[e] = cscale(G, beta);
        gb[e] = g + cscale(cscale(g, L), mu);
    }
}
template <typename T>
static int stage_update_impl(const void* f, const void* hp, const void* b, const void* Lt, const double* c, void* h, void* u,
                             long batch, long plane, hipStream_t st) {
    const long total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_stage_update<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)f, (const cx<T>*)hp, (const cx<T>*)b,
                       (const T*)Lt, (T)c[0], (T)c[1], (T)c[2], (T)c[3], (T)c[4], (cx<T>*)h, (cx<T>*)u, total, plane);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <typename T>
static int stage_update_vjp_impl(const void* gu, const void* gh, const void* Lt, const double* c, void* gf, void* ghp, void* gb,
                                 long batch, long plane, hipStream_t st) {
    const long total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_stage_update_vjp<T>, dim3(blocks), dim3(256), 0, st, (const cx<T>*)gu, (const cx<T>*)gh, (const T*)Lt,
                       (T)c[0], (T)c[1], (T)c[2], (T)c[3], (T)c[4], (cx<T>*)gf, (cx<T>*)ghp, (cx<T>*)gb, total, plane);
    HIP_TRY(hipGetLastError());
    return 0;
}
// coef = {fa, beta, gdt, mu, mud}
extern "C" int tcfd_ns2d_stage_update(const void* f, const void* h_prev, const void* b, const void* lin, const double* coef,
                                    void* h, void* u, long batch, long plane, int dtype, void* stream) {
    if (!f || !b || !lin || !coef || !h || !u || batch <= 0 || plane <= 0) return fail(TCFD_EINVAL, "stage_update: bad argument");
    if (dtype == TCFD_C128) return stage_update_impl<double>(f, h_prev, b, lin, coef, h, u, batch, plane, (hipStream_t)stream);
    if (dtype == TCFD_C64) return stage_update_impl<float>(f, h_prev, b, lin, coef, h, u, batch, plane, (hipStream_t)stream);
    return fail(TCFD_EINVAL, "stage_update: bad dtype %d", dtype);
}
extern "C" int tcfd_ns2d_stage_update_vjp(const void* g_u, const void* g_h, const void* lin, const double* coef, void* g_f,
                                        void* g_hprev, void* g_b, long batch, long plane, int dtype, void* stream) {
    if (!g_u || !lin || !coef || !g_f || !g_b || batch <= 0 || plane <= 0) return fail(TCFD_EINVAL, "stage_update_vjp: bad argument");
    if (dtype == TCFD_C128)
        return stage_update_vjp_impl<double>(g_u, g_h, lin, coef, g_f, g_hprev, g_b, batch, plane, (hipStream_t)stream);
    if (dtype == TCFD_C64)
        return stage_update_vjp_impl<float>(g_u, g_h, lin, coef, g_f, g_hprev, g_b, batch, plane, (hipStream_t)stream);
    return fail(TCFD_EINVAL, "stage_update_vjp: bad dtype %d", dtype);
}

// wbar = sum_f post_f (.) X_f : the last step of the explicit terms' vector-Jacobian product (X: (4, batch, plane) half spectra
// from tcfd_ns2d_explicit_terms_vjp, post: (4, plane) complex tables -(c / n^2) conj(a_f)).  As tensor ops this was a broadcast
// multiply writing 4 planes per field and a reduction reading them back (0.34 ms per stage at 1024^2 x 8); one pass here.
template <typename T>
__global__ __launch_bounds__(256) void k_vjp_combine(const cx<T>* __restrict__ X, const cx<T>* __restrict__ post,
                                                     cx<T>* __restrict__ out, long total, long plane) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256L) {
        const long t = e % plane;
        cx<T> acc = mk<T>((T)0, (T)0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const cx<T> x = X[(long)f * total + e], p = post[(long)f * plane + t];
            acc = acc + mk<T>(x.x * p.x - x.y * p.y, x.x * p.y + x.y * p.x);
        }
        out[e] = acc;
    }
}
extern "C" int tcfd_ns2d_vjp_combine(const void* X, const void* post, void* out, long batch, long plane, int dtype, void* stream) {
    if (!X || !post || !out || batch <= 0 || plane <= 0) return fail(TCFD_EINVAL, "vjp_combine: bad argument");
    const long total = batch * plane;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 1 << 16);
    if (dtype == TCFD_C128)
        hipLaunchKernelGGL(k_vjp_combine<double>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const cx<double>*)X,
                           (const cx<double>*)post, (cx<double>*)out, total, plane);
    else if (dtype == TCFD_C64)
        hipLaunchKernelGGL(k_vjp_combine<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const cx<float>*)X,
                           (const cx<float>*)post, (cx<float>*)out, total, plane);
    else
        return fail(TCFD_EINVAL, "vjp_combine: bad dtype %d", dtype);
    HIP_TRY(hipGetLastError());
    return 0;
}
